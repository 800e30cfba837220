"""GPU: exact filtered Flat search over a row mask (GpuIndex.make_mask / flat_knn_filtered / range_search(mask=...)) against the
CPU oracle.

The expected answer of a query comes from the oracle as it stands: oracle.flat_knn_batch(base, qs, len(base), kind) -- every row in
the reference's (distance, index) order -- keeping the pairs whose id is allowed and taking the first k (range: cutting at the radius
and the limit).  Every case is bit-exact: ids equal, distances equal as f32 bit patterns, counts / CSR offsets equal, slots past the
count zero.  A 3000-row table takes the direct path (gathered strict-order scan); a 30 000-row table in mode 2 runs the 8-bit tier with
the masked row constants, and mode 1 (direct everywhere) must agree with it."""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries")
KSTATS = ("flat_i8_queries", "flat_i8_redo", "flat_half_queries")


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


# ---- direct path ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """3000 x 960 gist-like rows, 9 queries (one group of 8 plus one), both metrics' full orders"""
    base = gist_like(3000, seed=2101)
    qs = gist_like(9, seed=2102)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


def _small_masks(n):
    rng = np.random.default_rng(5)
    return {
        "random30": rng.random(n) < 0.3,
        "one": _allow(n, [1234]),
        "last": _allow(n, [n - 1]),
        "first64": _allow(n, range(64)),
        "all": np.ones(n, dtype=np.bool_),
        "none": np.zeros(n, dtype=np.bool_),
    }


@pytest.mark.parametrize("dist,kind", DISTS)
def test_direct_path_masks_and_k(small, dist, kind):
    base, qs, fulls = small
    full = fulls[kind]
    ix = _index(dist, base)
    try:
        for name, allow in _small_masks(len(base)).items():
            mk = ix.make_mask(allow)
            try:
                assert len(mk) == int(allow.sum())
                for k in (1, 10, 64, 100, 2000):  # 2000 > 1024: the sort route wherever m > 1024, and > m for most masks
                    s0 = _stats(ix)
                    got = ix.flat_knn_filtered(qs, k, mk)
                    _same_knn(got, _expect_knn(full, allow, k), (dist, name, k))
                    d = _delta(ix, s0)
                    assert d["flat_filtered_queries"] == len(qs) and d["flat_filtered_direct_queries"] == len(qs), d
                    assert d["flat_filtered_i8_queries"] == 0 and d["flat_filtered_fallback_queries"] == 0, d
                # one query: the first `count` pairs
                gi, gd = ix.flat_knn_filtered(qs[4], 10, mk)
                ei, ed, ec = _expect_knn((full[0][4:5], full[1][4:5]), allow, 10)
                assert np.array_equal(gi, ei[0, : int(ec[0])]) and np.array_equal(gd.view(np.uint32), ed[0, : int(ec[0])].view(np.uint32))
                # k == 0 and no queries
                gi0, gd0, gc0 = ix.flat_knn_filtered(qs, 0, mk)
                assert gi0.shape == (len(qs), 0) and not gc0.any()
                assert ix.flat_knn_filtered(qs[:0], 5, mk)[2].shape == (0,)
            finally:
                mk.close()
    finally:
        ix.close()


def test_direct_path_id_offset(small):
    base, qs, fulls = small
    ix = _index("l2sqr", base)
    allow = _small_masks(len(base))["random30"]
    try:
        ix.set_id_offset(1000)
        mk = ix.make_mask(allow)  # LOCAL rows; the offset is added to what is reported
        _same_knn(ix.flat_knn_filtered(qs, 10, mk), _expect_knn(fulls[0], allow, 10, id_offset=1000), "id offset")
        _same_knn(ix.flat_knn_filtered(qs, 1500, mk), _expect_knn(fulls[0], allow, 1500, id_offset=1000), "id offset, sort route")
        mk.close()
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_direct_path_dim_not_multiple_of_4(dist, kind):
    rng = np.random.default_rng(30)
    base = rng.standard_normal((500, 30)).astype(np.float32)
    qs = rng.standard_normal((9, 30)).astype(np.float32)
    full = _full_order(base, qs, kind)
    allow = rng.random(500) < 0.5
    ix = _index(dist, base)
    try:
        mk = ix.make_mask(np.flatnonzero(allow))  # (an id list this time)
        for k in (1, 7, 600):
            _same_knn(ix.flat_knn_filtered(qs, k, mk), _expect_knn(full, allow, k), (dist, k))
        mk.close()
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_direct_path_nan_zero_and_duplicate_rows(dist, kind):
    rng = np.random.default_rng(31)
    base = rng.random((300, 64)).astype(np.float32)
    base[5, 17] = np.nan       # NaN distance to every query: sorts last
    base[9] = 0.0              # Cosine: the clamp of the denominator
    base[20:30] = base[3]      # ties, decided by id
    qs = np.concatenate([rng.random((8, 64)).astype(np.float32), base[3:4]])
    full = _full_order(base, qs, kind)
    ids = np.concatenate([[3, 5, 9], np.arange(20, 30), rng.choice(np.arange(40, 300), 50, replace=False)])
    allow = _allow(300, ids)
    m = int(allow.sum())
    ix = _index(dist, base)
    try:
        mk = ix.make_mask(allow)
        for k in (1, 11, m - 1, m, m + 5):
            got = ix.flat_knn_filtered(qs, k, mk)
            _same_knn(got, _expect_knn(full, allow, k), (dist, k))
        gi, gd, gc = ix.flat_knn_filtered(qs, m, mk)
        assert (gi[:, m - 1] == 5).all() and np.isnan(gd[:, m - 1]).all()  # the NaN row only when k >= m, last
        gi, gd, gc = ix.flat_knn_filtered(qs, m - 1, mk)
        assert not (gi == 5).any()
        gi, _, _ = ix.flat_knn_filtered(qs[8:9], 11, mk)
        assert list(gi[0]) == [3] + list(range(20, 30))  # the query IS row 3: eleven equal rows in id order
        mk.close()
    finally:
        ix.close()


# ---- 8-bit tier -------------------------------------------------------------------------------------------------------------------------
NB = 30000


@pytest.fixture(scope="module")
def big():
    """30 000 x 960 gist-like rows, 130 queries (two groups of 128, the second mostly padding), both metrics' full orders"""
    base = gist_like(NB, seed=2201)
    qs = gist_like(130, seed=2202)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}


def _big_masks():
    rng = np.random.default_rng(6)
    return {
        "m15000": _allow(NB, rng.choice(NB, 15000, replace=False)),
        "m8193": _allow(NB, rng.choice(NB, 8193, replace=False)),  # one row past the direct path's default domain
        "clustered": _allow(NB, range(10000, 20000)),              # whole units of the mirror without an allowed row
    }


@pytest.mark.parametrize("dist,kind", DISTS)
def test_tier_against_oracle_and_direct(big, dist, kind):
    base, qs, fulls = big
    full = fulls[kind]
    ix = _index(dist, base, 2)
    try:
        for name, allow in _big_masks().items():
            mk = ix.make_mask(allow)
            for k in (1, 10, 64):
                exp = _expect_knn(full, allow, k)
                ix.set_flat_mode(2)
                s0 = _stats(ix)
                got_t = ix.flat_knn_filtered(qs, k, mk)
                d = _delta(ix, s0)
                print(dist, name, k, d)
                _same_knn(got_t, exp, (dist, name, k, "tier"))
                assert d["flat_filtered_i8_queries"] == len(qs) == 130, d
                assert d["flat_filtered_direct_queries"] + d["flat_filtered_i8_queries"] == d["flat_filtered_queries"], d
                assert d["flat_filtered_fallback_queries"] <= len(qs)
                ix.set_flat_mode(1)  # direct everywhere
                s0 = _stats(ix)
                got_d = ix.flat_knn_filtered(qs, k, mk)
                d = _delta(ix, s0)
                _same_knn(got_d, exp, (dist, name, k, "direct"))
                _same_knn(got_t, got_d, (dist, name, k, "tier vs direct"))
                assert d["flat_filtered_direct_queries"] == len(qs) and d["flat_filtered_i8_queries"] == 0, d
            mk.close()
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_tier_threshold_clamp(big, dist, kind):
    """Allow-lists so short that the threshold sample holds fewer allowed rows than its rank (m = 40: every sampled key but 40 is +inf, the
    selected threshold is +inf) or barely enough (m = 300).  Unclamped, +inf would admit every masked row.  Clamped, the query collects its
    allowed rows; 40 of them fit one round of the walk and the list is exhausted below a threshold of FLT_MAX, so nothing is handed on."""
    base, qs, fulls = big
    full = fulls[kind]
    rng = np.random.default_rng(7)
    ix = _index(dist, base, 2)
    try:
        ix.set_param("flat_filtered_direct_max", 0)
        for m in (300, 40):
            allow = _allow(NB, rng.choice(NB, m, replace=False))
            mk = ix.make_mask(allow)
            for k in (10, 64):
                s0 = _stats(ix)
                got = ix.flat_knn_filtered(qs, k, mk)
                d = _delta(ix, s0)
                print(dist, m, k, d)
                _same_knn(got, _expect_knn(full, allow, k), (dist, m, k))
                assert d["flat_filtered_i8_queries"] == len(qs), d
                if m == 40:
                    assert d["flat_filtered_fallback_queries"] == 0, d
            mk.close()
    finally:
        ix.close()


def test_tier_hands_on_a_tight_cluster():
    """600 allowed near-copies of one row, all inside the 8-bit keys' resolution of each other: the walk (limited to 256 rows here) cannot
    separate the k-th from the rest of the cluster, the queries next to it are handed to the direct path, and the answer is still exact."""
    rng = np.random.default_rng(8)
    base = gist_like(NB, seed=2301)
    centre = base[77].copy()
    near = np.round(np.clip(np.abs(centre + rng.standard_normal((600, 960)).astype(np.float32) * np.float32(2e-4)), 0, 0.8), 4).astype(np.float32)
    base[1000:1600] = near
    qs = np.concatenate([near[:4] + np.float32(1e-4), gist_like(4, seed=2302)]).astype(np.float32)
    full = _full_order(base, qs, 0)
    allow = rng.random(NB) < 0.5
    allow[1000:1600] = True
    ix = _index("l2sqr", base, 2)
    try:
        ix.set_param("flat_i8_rows", 256)
        mk = ix.make_mask(allow)
        s0 = _stats(ix)
        got = ix.flat_knn_filtered(qs, 10, mk)
        d = _delta(ix, s0)
        print(d)
        _same_knn(got, _expect_knn(full, allow, 10), "tight cluster")
        assert d["flat_filtered_i8_queries"] == len(qs) and d["flat_filtered_fallback_queries"] > 0, d
        mk.close()
    finally:
        ix.close()


def test_many_queries_cross_the_tier_rounds():
    """More queries than one round of the tier takes (1024): output offsets, per-round flags and the hand-on indices across the seam.  300
    allowed near-copies of one row with queries next to them on both sides of query 1024 (walk limited to 256 rows): both rounds hand on."""
    rng = np.random.default_rng(10)
    base = gist_like(17000, dim=128, seed=2401)
    centre = base[77].copy()
    near = np.round(np.clip(np.abs(centre + rng.standard_normal((300, 128)).astype(np.float32) * np.float32(2e-4)), 0, 0.8), 4).astype(np.float32)
    base[1000:1300] = near
    qs = gist_like(1100, dim=128, seed=2402)
    at = np.array([3, 500, 1023, 1024, 1025, 1099])  # queries next to the cluster, in the first round and in the second
    qs[at] = near[: len(at)] + np.float32(1e-4)
    allow = rng.random(17000) < 0.5
    allow[1000:1300] = True
    exp = _expect_knn(_full_order(base, qs, 0), allow, 10)
    assert np.isin(exp[0][at], np.arange(1000, 1300)).all()  # (the cluster queries' neighbours ARE the cluster)
    ix = _index("l2sqr", base, 2)
    try:
        ix.set_param("flat_filtered_direct_max", 0)
        ix.set_param("flat_i8_rows", 256)
        mk = ix.make_mask(allow)
        s0 = _stats(ix)
        got_t = ix.flat_knn_filtered(qs, 10, mk)
        d = _delta(ix, s0)
        print(d)
        _same_knn(got_t, exp, "1100 queries: tier")
        assert d["flat_filtered_i8_queries"] == 1100 and d["flat_filtered_fallback_queries"] > 0, d
        ix.set_flat_mode(1)
        _same_knn(got_t, ix.flat_knn_filtered(qs, 10, mk), "1100 queries: tier vs direct")
        mk.close()
    finally:
        ix.close()


def test_unfiltered_search_is_isolated(big):
    """an unfiltered flat_knn before and after filtered calls returns identical bits, and the k-NN tiers' counters move only by it"""
    base, qs, fulls = big
    masks = _big_masks()
    ix = _index("l2sqr", base, 2)
    try:
        s0 = _stats(ix, KSTATS)
        a = ix.flat_knn(qs, 10)
        s1 = _stats(ix, KSTATS)
        mk, mk2 = ix.make_mask(masks["m15000"]), ix.make_mask(_allow(NB, range(100)))
        ix.flat_knn_filtered(qs, 10, mk)    # tier
        ix.flat_knn_filtered(qs, 10, mk2)   # direct
        ix.range_search(qs[:8], fulls[0][1][:8, 9], mask=mk)
        s2 = _stats(ix, KSTATS)
        assert s2 == s1, (s1, s2)
        b = ix.flat_knn(qs, 10)
        s3 = _stats(ix, KSTATS)
        _same_knn(a, b, "unfiltered before / after")
        _same_knn(a, _expect_knn(fulls[0], np.ones(NB, dtype=np.bool_), 10), "unfiltered vs oracle")
        assert {s: s3[s] - s2[s] for s in KSTATS} == {s: s1[s] - s0[s] for s in KSTATS}
        mk.close()
        mk2.close()
    finally:
        ix.close()


def test_concurrent_first_use_of_a_mask(big):
    """four threads issue the first tier call on one fresh mask at once (the lazy build of the masked row constants)"""
    base, qs, fulls = big
    allow = _big_masks()["m15000"]
    exp = _expect_knn(fulls[0], allow, 10)
    ix = _index("l2sqr", base, 2)
    try:
        ix.flat_knn(qs[:8], 10)  # (the mirror itself is built; the mask's copy is not)
        mk = ix.make_mask(allow)
        out, errs = [None] * 4, []
        bar = threading.Barrier(4)

        def work(t):
            try:
                bar.wait()
                out[t] = ix.flat_knn_filtered(qs, 10, mk)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for t in range(4):
            _same_knn(out[t], exp, ("thread", t))
        mk.close()
    finally:
        ix.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_mask_errors(small):
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.index import RowMask, pack_mask

    base, qs, _ = small
    ix, other = _index("l2sqr", base[:500]), _index("l2sqr", base[:500])
    try:
        with pytest.raises(vdb.VdbError, match="error 1"):  # wrong length
            RowMask(ix, pack_mask(np.ones(505, dtype=np.bool_), 505), 505)
        mk = other.make_mask(np.ones(500, dtype=np.bool_))
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.flat_knn_filtered(qs, 5, mk)
        with pytest.raises(vdb.VdbError, match="error 1.*another index"):
            ix.range_search(qs, 1.0, mask=mk)
        mk.close()
        mk = ix.make_mask(np.ones(500, dtype=np.bool_))
        ix.flat_knn_filtered(qs, 5, mk)
        ix.batch_add(base[500:510])
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 5, mk)
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.range_search(qs, 1.0, mask=mk)
        mk.close()
        mk = ix.make_mask(np.ones(510, dtype=np.bool_))
        ix.flat_knn_filtered(qs, 5, mk)
        ix.swap_remove(3)
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 5, mk)
        mk.close()
        ix.batch_add(base[600:601])  # the same length as when the mask was made: still stale
        assert len(ix) == 510
        mk2 = ix.make_mask(np.ones(510, dtype=np.bool_))
        ix.swap_remove(0)
        ix.batch_add(base[601:602])
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_filtered(qs, 5, mk2)
        mk2.close()
    finally:
        ix.close()
        other.close()
    u8 = vdb.GpuIndex(64, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.random.default_rng(1).integers(0, 256, (100, 64), dtype=np.uint8))
        mk = u8.make_mask(np.ones(100, dtype=np.bool_))
        with pytest.raises(vdb.VdbError, match="error 1.*f32 rows"):
            u8.flat_knn_filtered(np.zeros((2, 64), dtype=np.float32), 5, mk)
        mk.close()
    finally:
        u8.close()


# ---- range ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,kind", DISTS)
def test_filtered_range_tier_and_scan(big, dist, kind):
    base, qs, fulls = big
    qs = qs[:24]
    full = (fulls[kind][0][:24], fulls[kind][1][:24])
    masks = _big_masks()
    tier, scan = _index(dist, base, 2), _index(dist, base, 1)
    try:
        for name in ("m15000", "clustered"):
            allow = masks[name]
            mt, ms = tier.make_mask(allow), scan.make_mask(allow)
            kth10 = _expect_knn(full, allow, 10)[1][:, 9]
            radii = {"unfiltered64": full[1][:, 63].copy(), "below_allowed10": np.nextafter(kth10, np.float32(-np.inf))}
            for rname, r in radii.items():
                for limit in (None, 5):
                    exp = _expect_range(full, allow, r, limit)
                    got_t = tier.range_search(qs, r, limit, mask=mt)
                    got_s = scan.range_search(qs, r, limit, mask=ms)
                    _same_range(got_t, exp, (dist, name, rname, limit, "tier"))
                    _same_range(got_s, exp, (dist, name, rname, limit, "scan"))
            assert int(_expect_range(full, allow, radii["below_allowed10"])[0][-1]) >= 9 * 24 - 24  # (not vacuous: about nine pairs per query)
            mt.close()
            ms.close()
        # mask=None is the unfiltered call, bit for bit; a mask of every row gives the same
        r = full[1][:, 63].copy()
        every = np.ones(NB, dtype=np.bool_)
        exp = _expect_range(full, every, r)
        m_all = tier.make_mask(every)
        _same_range(tier.range_search(qs, r), exp, "unfiltered")
        _same_range(tier.range_search(qs, r, mask=None), exp, "mask=None")
        _same_range(tier.range_search(qs, r, mask=m_all), exp, "all rows")
        m_all.close()
    finally:
        tier.close()
        scan.close()


def test_filtered_range_u8_index():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(9)
    rows = rng.integers(0, 256, (2000, 64), dtype=np.uint8)
    qs = rng.integers(0, 256, (9, 64)).astype(np.float32)
    full = _full_order(rows.astype(np.float32), qs, 0)
    allow = rng.random(2000) < 0.4
    ix = vdb.GpuIndex(64, "l2sqr", scalar="u8")
    try:
        ix.batch_add_u8(rows)
        mk = ix.make_mask(allow)
        r = full[1][:, 63].copy()
        _same_range(ix.range_search(qs, r, mask=mk), _expect_range(full, allow, r), "u8 scan")
        _same_range(ix.range_search(qs, r, 7, mask=mk), _expect_range(full, allow, r, 7), "u8 scan, limit")
        mk.close()
    finally:
        ix.close()
