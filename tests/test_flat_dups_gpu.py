"""GPU: the near-duplicate grouping end to end (GpuIndex.dup_groups / dup_groups_device; vdb_flat_dup_groups) against tests/dup_ref.py.

Small tables on the scan route are compared with dup_ref over the lists derived from the oracle's pair distances (every row as a query
against every row, in the reference's order); the planted-copy tables (20 000 x 128; tests/test_dup_ref_cpu.py verifies their margins)
with dup_ref over the lists the existing range_search returns for the same rows as queries, and with the planted truth.  `group` and
`stats` are compared exactly."""
import threading

import numpy as np
import pytest

import dup_ref as R

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
NONE = R.ROW_NONE
DUP_STATS = ("flat_dup_calls", "flat_dup_chunks", "flat_dup_pairs")
RANGE_STATS = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_results")


def _index(dist, base, mode=None, u8=False):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist, device=0, scalar="u8" if u8 else "f32")
    if u8:
        ix.batch_add_u8(base)
    else:
        ix.batch_add(base)
    if mode is not None:
        ix.set_flat_mode(mode)
    return ix


def _small_table(dim, seed):
    """300 rows: random rows, four identical rows, two more identical ones far apart in the table, a near pair, a NaN row, a zero row"""
    rng = np.random.default_rng(seed)
    x = rng.random((300, dim), dtype=np.float32)
    x[[5, 17, 150, 299]] = x[5]
    x[[64, 191]] = x[64]
    x[100] = x[99] + np.float32(1e-3)
    x[200] = np.nan
    x[250] = 0.0
    return x


def _full_order(base, kind):
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, base, len(base), kind, nthreads=16)
    return oi.astype(np.int64), od


def _lists(full, radius, allowed=None):
    """(src, lists) by the rule: for every allowed row its allowed rows with D <= radius, in the oracle's order"""
    oi, od = full
    ok = np.ones(len(oi), dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    src, lists = [], []
    for i in np.flatnonzero(ok).tolist():
        with np.errstate(invalid="ignore"):
            inside = (od[i] <= np.float32(radius)) & ok[oi[i]]
        src.append(i)
        lists.append(oi[i][inside].tolist())
    return src, lists


def _expect(n, src, lists, allowed=None, limit=0, id_offset=0):
    lims, ids = R.csr(lists)
    return R.dup_ref(n, src, lims, ids, allowed, limit, id_offset)


def _same(got, exp, what=""):
    assert got[1] == exp[1], (what, got[1], exp[1])
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0]), (what, np.flatnonzero(got[0] != exp[0])[:8])


@pytest.fixture(scope="module")
def small():
    """dim -> (table, {kind: full order}), computed once and never changed"""
    out = {}
    for dim in (5, 20):
        x = _small_table(dim, 40 + dim)
        out[dim] = (x, {kind: _full_order(x, kind) for _, kind in DISTS})
    return out


@pytest.mark.parametrize("dim", (5, 20))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_small_tables_against_the_oracle(small, dim, dist, kind):
    x, fulls = small[dim]
    full = fulls[kind]
    n = len(x)
    ix = _index(dist, x)
    try:
        d_sorted = np.sort(full[1][np.isfinite(full[1])])
        radii = [0.0, -1.0, -np.inf, np.inf, float(d_sorted[n + 40]), float(d_sorted[3 * n]), float(d_sorted[len(d_sorted) // 20])]
        for r in radii:
            src, lists = _lists(full, r)
            got = ix.dup_groups(r)
            _same(got, _expect(n, src, lists), (dist, dim, r))
        g0, s0 = ix.dup_groups(0.0)
        if kind == 0:  # identical rows are linked at radius 0, wherever they lie; nothing else is
            assert g0[[5, 17, 150, 299]].tolist() == [5] * 4 and g0[[64, 191]].tolist() == [64] * 2 and s0["groups"] == 2 and s0["rows"] == 6
        assert g0[200] == 200 and ix.dup_groups(np.inf)[0][200] == 200  # the NaN row is alone at every radius
        gn, sn = ix.dup_groups(-1.0)
        assert np.array_equal(gn, np.arange(n, dtype=np.uint64)) and sn == {"groups": 0, "rows": 0, "pairs": 0, "truncated": 0}
        gi, si = ix.dup_groups(np.inf)  # ONE group: every row that has a distance to anything, under the lowest of them
        assert si["groups"] == 1 and si["rows"] >= n - 2 and (gi[[0, 1, 299]] == 0).all()
    finally:
        ix.close()


def test_chunk_boundary_five_chunks_against_one(small):
    x, fulls = small[5]
    ix = _index("l2sqr", x)
    try:
        r = float(np.sort(fulls[0][1][np.isfinite(fulls[0][1])])[3 * len(x)])
        one = ix.dup_groups(r)
        c0 = ix.get_stat("flat_dup_chunks")
        ix.set_param("flat_dup_chunk", 64)
        five = ix.dup_groups(r)
        assert ix.get_stat("flat_dup_chunks") - c0 == 5  # 300 rows: 64 + 64 + 64 + 64 + 44
        _same(five, one, "chunk 64 against one chunk")
        ix.set_param("flat_dup_chunk", 1)
        _same(ix.dup_groups(r), one, "chunk 1")
        ix.set_param("flat_dup_chunk", 299)
        _same(ix.dup_groups(r), one, "chunk 299")
        import lab_1806_vec_db_amd as vdb

        for bad in (0, -1, 2**20 + 1):
            with pytest.raises(vdb.VdbError):
                ix.set_param("flat_dup_chunk", bad)
    finally:
        ix.close()


def test_masks_from_both_constructors(small):
    x, fulls = small[20]
    full = fulls[0]
    n = len(x)
    ix = _index("l2sqr", x)
    try:
        rng = np.random.default_rng(8)
        r = float(np.sort(full[1][np.isfinite(full[1])])[3 * n])
        allow = rng.random(n) < 0.6
        allow[[5, 150, 299, 64, 191]] = True
        allow[17] = False
        ix.set_labels(0, np.where(allow, 1, 2).astype(np.uint32))
        ix.set_param("flat_dup_chunk", 64)
        for mk in (ix.make_mask(allow), ix.make_mask_where([(0, 1)])):
            for radius in (0.0, r, np.inf):
                src, lists = _lists(full, radius, allow)
                got = ix.dup_groups(radius, mask=mk)
                _same(got, _expect(n, src, lists, allow), ("mask", radius))
                assert (got[0][~allow] == NONE).all() and (got[0][allow] != NONE).all()
            mk.close()
        # a mask that excludes a chain's middle row: 0 - 1 - 2 along one axis, ends farther apart than the radius
        y = np.zeros((6, 20), dtype=np.float32)
        y[:, 1] = np.arange(6) * 10.0
        y[[0, 1, 2], 1] = [100.0, 101.0, 102.0]
        ch = _index("l2sqr", y)
        try:
            g, s = ch.dup_groups(1.0)
            assert g.tolist() == [0, 0, 0, 3, 4, 5] and s == {"groups": 1, "rows": 3, "pairs": 4, "truncated": 0}  # single linkage: D(0, 2) = 4
            mk = ch.make_mask(np.array([1, 0, 1, 1, 1, 1], dtype=bool))
            g, s = ch.dup_groups(1.0, mask=mk)
            assert g.tolist() == [0, NONE, 2, 3, 4, 5] and s == {"groups": 0, "rows": 0, "pairs": 0, "truncated": 0}  # a disallowed row never bridges
            mk.close()
        finally:
            ch.close()
    finally:
        ix.close()


def test_limit_on_identical_rows():
    x = np.random.default_rng(2).random((1200, 8), dtype=np.float32)
    x[100:1100] = x[100]
    ix = _index("l2sqr", x)
    try:
        # every one of the 1000 identical rows lists the 8 lowest of them: one group, 1000 truncated lists
        src = list(range(1200))
        lists = [list(range(100, 1100)) if 100 <= i < 1100 else [i] for i in src]
        exp = _expect(1200, src, lists, limit=8)
        got = ix.dup_groups(0.0, limit=8)
        _same(got, exp, "limit 8")
        assert got[1] == {"groups": 1, "rows": 1000, "pairs": 8 * 1000 - 8, "truncated": 1000}
        full = ix.dup_groups(0.0)
        assert full[1]["pairs"] == 1000 * 999 and full[1]["truncated"] == 0
        # the subset property on a table where the cut matters: a group under a limit lies inside one unlimited group
        y = np.random.default_rng(3).random((400, 3), dtype=np.float32)
        iy = _index("l2sqr", y)
        try:
            r = 0.02
            unl, _ = iy.dup_groups(r)
            for lim in (1, 2, 3):
                cut, st = iy.dup_groups(r, limit=lim)
                assert st["truncated"] > 0
                for rep in np.unique(cut).tolist():
                    assert len(set(unl[cut == rep].tolist())) == 1, (lim, rep)
            assert iy.dup_groups(r, limit=1)[1]["groups"] == 0  # a list of one entry is the row itself
            with pytest.raises(ValueError):
                iy.dup_groups(r, limit=0)
        finally:
            iy.close()
    finally:
        ix.close()


@pytest.fixture(scope="module")
def planted():
    """kind -> (table, radius, truth, range lists of every row as a query: (lims, ids)); the lists come from ONE range_search call on an
    index in its default mode and are shared by the cases below"""
    out = {}
    for kind in ("f32", "u8"):
        x, radius, truth, pairs, chains = R.planted_table(20000, 128, kind, R.PLANTED_SEEDS[kind])
        ix = _index("l2sqr", x, u8=kind == "u8")
        try:
            lims, ids, _ = ix.range_search(x.astype(np.float32), radius)
        finally:
            ix.close()
        out[kind] = (x, radius, truth, lims, ids, chains)
    return out


def _planted_expect(p):
    x, radius, truth, lims, ids, chains = p
    n = len(x)
    lists = [ids[int(lims[q]):int(lims[q + 1])].tolist() for q in range(n)]
    return _expect(n, list(range(n)), lists)


@pytest.mark.parametrize("kind,mode", (("f32", 1), ("f32", 2), ("u8", None)))
def test_planted_copies(planted, kind, mode):
    p = planted[kind]
    x, radius, truth = p[0], p[1], p[2]
    exp = _planted_expect(p)
    assert np.array_equal(exp[0], truth.astype(np.uint64)) and exp[1]["groups"] == 200  # the reference finds the planted groups
    ix = _index("l2sqr", x, mode=mode, u8=kind == "u8")
    try:
        before = {s: ix.get_stat(s) for s in DUP_STATS + RANGE_STATS}
        got = ix.dup_groups(radius)
        _same(got, exp, (kind, mode))
        assert np.array_equal(got[0], truth.astype(np.uint64))
        after = {s: ix.get_stat(s) for s in DUP_STATS + RANGE_STATS}
        d = {s: after[s] - before[s] for s in after}
        n = len(x)
        assert d["flat_dup_calls"] == 1 and d["flat_dup_chunks"] == -(-n // 16384) and d["flat_dup_pairs"] == got[1]["pairs"]
        assert d["flat_range_queries"] == n and d["flat_range_results"] == got[1]["pairs"] + n  # every row lists itself
        assert d["flat_range_i8_queries"] + d["flat_range_scan_queries"] == n
        if mode == 1 or kind == "u8":
            assert d["flat_range_i8_queries"] == 0
        if mode == 2:
            assert d["flat_range_i8_queries"] > 0  # the tier ran (how many rows it kept is reported by the bench, not gated)
        # a chain's ends are one group although they are farther apart than the radius
        c = max(p[5], key=len)
        assert len(c) >= 3 and got[0][c[0]] == got[0][c[-1]] == min(c)
    finally:
        ix.close()


def test_device_form_id_offset_and_counters(planted):
    import torch

    import lab_1806_vec_db_amd as vdb

    x, radius, truth = planted["f32"][:3]
    sub = x[:3000]
    ix = _index("l2sqr", sub)
    try:
        host = ix.dup_groups(radius)
        out = torch.full((len(sub),), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = ix.dup_groups_device(radius, out.data_ptr())
        torch.cuda.synchronize()
        _same((out.cpu().numpy().view(np.uint64), st), host, "device form")
        ix.set_id_offset(1 << 33)
        off = ix.dup_groups(radius)
        assert off[1] == host[1] and np.array_equal(off[0], host[0] + np.uint64(1 << 33))
        ix.set_id_offset(0)
        # refusals: the output (sentinel-filled) and the new counters stay as found
        other = _index("l2sqr", sub[:100])
        stale_ix = _index("l2sqr", sub[:100])
        try:
            foreign = other.make_mask(np.ones(100, dtype=bool))
            stale = stale_ix.make_mask(np.ones(100, dtype=bool))
            stale_ix.batch_add(sub[100:101])
            before = [ix.get_stat(s) for s in DUP_STATS]
            out.fill_(-7)
            torch.cuda.synchronize()
            with pytest.raises(vdb.VdbError, match="NaN"):
                ix.dup_groups_device(float("nan"), out.data_ptr())
            with pytest.raises(vdb.VdbError, match="another index"):
                ix.dup_groups_device(radius, out.data_ptr(), mask=foreign)
            with pytest.raises(vdb.VdbError, match="stale"):
                stale_ix.dup_groups(radius, mask=stale)
            with pytest.raises(vdb.VdbError):
                ix.dup_groups_device(radius, 0)
            # a chunk whose range call fails fails the whole call: +inf over 3000 rows is 9 000 000 pairs, past a ceiling of 1 000 000
            ix.set_param("flat_range_max_results", 1_000_000)
            ix.set_param("flat_dup_chunk", 1024)
            with pytest.raises(vdb.VdbError, match="flat_range_max_results"):
                ix.dup_groups_device(np.inf, out.data_ptr())
            ix.set_param("flat_range_max_results", 0)
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == -7).all()
            assert [ix.get_stat(s) for s in DUP_STATS] == before
            foreign.close()
            stale.close()
        finally:
            other.close()
            stale_ix.close()
        # an empty index
        e = vdb.GpuIndex(8, "l2sqr", device=0)
        g, s = e.dup_groups(1.0)
        assert g.shape == (0,) and s == {"groups": 0, "rows": 0, "pairs": 0, "truncated": 0}
        e.close()
    finally:
        ix.close()


def test_two_threads(planted):
    x, radius = planted["f32"][:2]
    sub = x[:6000]
    ix = _index("l2sqr", sub)
    try:
        ix.set_param("flat_dup_chunk", 1024)
        ref = ix.dup_groups(radius)
        mk = ix.make_mask(np.arange(len(sub)) % 3 != 0)
        ref_m = ix.dup_groups(radius, mask=mk)
        got, errs = {}, []

        def work(t):
            try:
                for it in range(3):
                    got[(t, it)] = ix.dup_groups(radius, mask=mk if t else None)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for (t, it), g in got.items():
            _same(g, ref_m if t else ref, ("thread", t, it))
        mk.close()
    finally:
        ix.close()
