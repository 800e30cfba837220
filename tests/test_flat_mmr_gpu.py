"""GPU: diversified Flat k-NN (GpuIndex.flat_knn_mmr, vdb_flat_knn_mmr: maximal marginal relevance over the fetch_k nearest allowed
rows) end to end against the CPU oracle.

The candidates of a query are the first min(fetch_k, m) entries of the oracle's full order -- oracle.flat_knn_batch(base, qs, len(base),
kind): every row in the reference's (distance, index) order, NaN distances last -- restricted to the rows the query's mask allows;
tests/mmr_ref.py (verified by tests/test_mmr_ref_cpu.py) selects from them over oracle.dist pair distances.  Every case is bit-exact:
ids equal in selection order, distances equal as f32 bit patterns, counts equal, slots past the count zero."""
import threading

import numpy as np
import pytest

import mmr_ref as R
from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
MSTATS = ("flat_mmr_calls", "flat_mmr_queries")
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries", "flat_fallback", "flat_i8_queries", "flat_half_queries",
          "flat_grouped_calls", "flat_grouped_queries")
# (k, fetch_k, lambda): the default shape, fetch_k == k, farthest-first, a list past the 8-bit tier's 64, one hit, lambda = 1
CASES = ((10, 40, 0.5), (10, 10, 0.5), (5, 64, 0.0), (10, 100, 0.25), (1, 1, 0.5), (1, 30, 0.75), (12, 40, 1.0))


def _full_order(base, qs, kind):
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.int64), od


def _random_set():
    rng = np.random.default_rng(5101)
    base = rng.random((2000, 64)).astype(np.float32)
    base[5, 17] = np.nan     # NaN distance to every query: last in every order, a candidate only when fetch_k reaches it
    base[20:30] = base[3]    # identical rows: D = 0 between them
    qs = np.concatenate([rng.random((7, 64)).astype(np.float32), base[3:4]])
    return base, qs


def _clustered_set():
    """20 clusters of 8 near-duplicates each (row r belongs to cluster r % 20): what the feature exists for -- the plain top 10 of a
    query near a centre is that cluster and two rows of the next, while 40 candidates reach five clusters"""
    rng = np.random.default_rng(5102)
    centres = rng.random((20, 64)).astype(np.float32)
    base = (centres[np.arange(160) % 20] + rng.standard_normal((160, 64)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    qs = (centres[:8] + rng.standard_normal((8, 64)).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    return base, qs


class Data:
    def __init__(self, base, qs):
        self.base, self.qs = base, qs
        self.full = {kind: _full_order(base, qs, kind) for _, kind in DISTS}
        self.rd = {kind: R.RowDist(base, kind) for _, kind in DISTS}

    def expect(self, kind, k, fetch_k, lam, allows=None, mask_of=None, id_offset=0, queries=None):
        oi, od = self.full[kind]
        qsel = range(len(oi)) if queries is None else queries
        kk = max(k, 1)
        idx = np.zeros((len(qsel), kk), dtype=np.uint64)
        dist = np.zeros((len(qsel), kk), dtype=np.float32)
        cnt = np.zeros(len(qsel), dtype=np.uint64)
        for j, q in enumerate(qsel):
            rows, d = oi[q], od[q]
            if allows is not None:
                keep = allows[int(mask_of[j])][rows]
                rows, d = rows[keep], d[keep]
            rows, d = rows[:fetch_k], d[:fetch_k]
            sel = R.walk_rows(self.rd[kind], rows, d, k, lam)
            cnt[j] = len(sel)
            idx[j, :len(sel)] = rows[sel].astype(np.uint64) + np.uint64(id_offset)
            dist[j, :len(sel)] = d[sel]
        return idx[:, :k], dist[:, :k], cnt


@pytest.fixture(scope="module")
def sets():
    """the three data sets with both metrics' full orders (computed once, never changed)"""
    return {"random": Data(*_random_set()), "gist": Data(gist_like(300, seed=5103), gist_like(6, seed=5104)), "clustered": Data(*_clustered_set())}


def _same(got, exp, what=""):
    gi, gd, gc = got
    ei, ed, ec = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), (what, gi[:2], ei[:2])
    assert gd.dtype == np.float32 and np.array_equal(np.isnan(gd), np.isnan(ed)), what  # (a NaN's payload is not part of the search's contract)
    ok = ~np.isnan(ed)
    assert np.array_equal(gd[ok].view(np.uint32), ed[ok].view(np.uint32)), what


def _stats(ix, names=MSTATS + FSTATS):
    return {s: ix.get_stat(s) for s in names}


def _delta(ix, s0):
    return {s: ix.get_stat(s) - v for s, v in s0.items()}


def _allow(n, ids):
    a = np.zeros(n, dtype=np.bool_)
    a[np.asarray(ids, dtype=np.int64)] = True
    return a


def _index(dist, base):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist)
    ix.batch_add(base)
    return ix


def test_the_clustered_reference_is_not_the_plain_search(sets):
    """on the CPU, before anything runs on the GPU: at lambda = 0.5 the reference's answer differs from the plain top k for most
    queries of the clustered set, so no test below can pass by returning the plain k-NN"""
    data = sets["clustered"]
    for _, kind in DISTS:
        ei, _, ec = data.expect(kind, 10, 40, 0.5)
        plain = data.full[kind][0][:, :10]
        differ = sum(ei[q].tolist() != plain[q].tolist() for q in range(len(ei)))
        assert (ec == 10).all() and differ >= 6, (kind, differ)
        if kind == 0:  # the answer reaches more clusters than the plain top 10 does
            assert np.mean([len(set((ei[q] % 20).tolist())) for q in range(len(ei))]) > np.mean([len(set((plain[q] % 20).tolist())) for q in range(len(ei))])


@pytest.mark.parametrize("name", ("random", "gist", "clustered"))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_cases_against_the_oracle(sets, name, dist, kind):
    data = sets[name]
    ix = _index(dist, data.base)
    nq = len(data.qs)
    try:
        for k, fk, lam in CASES:
            s0 = _stats(ix, MSTATS)
            got = ix.flat_knn_mmr(data.qs, k, fk, lam)
            d = _delta(ix, s0)
            _same(got, data.expect(kind, k, fk, lam), (name, dist, k, fk, lam))
            assert d == {"flat_mmr_calls": 1, "flat_mmr_queries": nq}, d
        # fetch_k past the table: every row is a candidate (the NaN row of the random set among them)
        k, fk = (12, 4096) if len(data.base) <= 300 else (4, 2000)
        for lam in (0.0, 0.5):
            got = ix.flat_knn_mmr(data.qs, k, fk, lam)
            _same(got, data.expect(kind, k, fk, lam), (name, dist, "every row", lam))
        # one query, as flat_knn returns one
        gi, gd = ix.flat_knn_mmr(data.qs[2], 10, 40, 0.5)
        ei, ed, _ = data.expect(kind, 10, 40, 0.5, queries=[2])
        assert np.array_equal(gi, ei[0]) and np.array_equal(gd.view(np.uint32), ed[0].view(np.uint32))
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_lambda_one_is_flat_knn_and_fetch_k_equal_k_permutes_it(sets, dist, kind):
    data = sets["random"]
    ix = _index(dist, data.base)
    try:
        for k in (1, 10, 64, 100):
            plain = ix.flat_knn(data.qs, k)
            _same(ix.flat_knn_mmr(data.qs, k, k, 1.0), plain, (dist, k, "lambda 1, fetch_k k"))
            _same(ix.flat_knn_mmr(data.qs, k, min(4 * k, 4096), 1.0), plain, (dist, k, "lambda 1"))
            gi, gd, gc = ix.flat_knn_mmr(data.qs, k, k, 0.3)
            assert np.array_equal(gc, plain[2]) and np.array_equal(np.sort(gi, axis=1), np.sort(plain[0], axis=1))
            assert (gi[:, 0] == plain[0][:, 0]).all()  # the nearest row comes first whatever lambda is
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_with_masks_on_both_routes(sets, dist, kind):
    """one mask for every query, and a mask per query -- an empty one, one shorter than k (m < k), one shorter than fetch_k, long ones --
    with the masks of up to "flat_filtered_direct_max" rows in the filtered call's one launch and the longer ones on its per-mask route"""
    data = sets["random"]
    n, nq = len(data.base), len(data.qs)
    rng = np.random.default_rng(8)
    allows = [_allow(n, rng.choice(n, 1200, replace=False)), _allow(n, []), _allow(n, rng.choice(n, 5, replace=False)),
              _allow(n, rng.choice(n, 30, replace=False)), np.ones(n, dtype=np.bool_), _allow(n, np.arange(0, n, 3))]
    ix = _index(dist, data.base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        zero = np.zeros(nq, dtype=np.uint32)
        mask_of = (np.arange(nq) * 5 % len(masks)).astype(np.uint32)
        for direct_max in (8192, 100):  # 100: the masks of 1200, 2000 and 667 rows leave the one launch
            ix.set_param("flat_filtered_direct_max", direct_max)
            for k, fk, lam in ((10, 40, 0.5), (10, 10, 0.0), (4, 100, 0.25)):
                s0 = _stats(ix)
                got = ix.flat_knn_mmr(data.qs, k, fk, lam, masks[0])
                d = _delta(ix, s0)
                _same(got, data.expect(kind, k, fk, lam, allows[:1], zero), (dist, direct_max, k, fk, lam, "one mask"))
                # the underlying search's counters advance as for vdb_flat_knn_filtered_multi at k = the list length
                s1 = _stats(ix)
                ix.flat_knn_filtered_multi(data.qs, fk, masks[:1], zero)
                d1 = _delta(ix, s1)
                assert d["flat_mmr_calls"] == 1 and d["flat_mmr_queries"] == nq and d1["flat_mmr_calls"] == 0
                assert {s: d[s] for s in FSTATS} == {s: d1[s] for s in FSTATS}, (d, d1)
                got = ix.flat_knn_mmr(data.qs, k, fk, lam, masks, mask_of)
                _same(got, data.expect(kind, k, fk, lam, allows, mask_of), (dist, direct_max, k, fk, lam, "mask per query"))
                assert (got[2][mask_of == 1] == 0).all() and (got[2][mask_of == 2] == min(k, 5)).all()
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_unfiltered_counters_advance_as_for_flat_knn(sets):
    data = sets["gist"]
    ix = _index("l2sqr", data.base)
    try:
        for fk in (40, 100):
            s0 = _stats(ix)
            ix.flat_knn_mmr(data.qs, 10, fk, 0.5)
            d = _delta(ix, s0)
            s1 = _stats(ix)
            ix.flat_knn(data.qs, fk)
            d1 = _delta(ix, s1)
            assert d["flat_mmr_calls"] == 1 and d["flat_mmr_queries"] == len(data.qs)
            assert {s: d[s] for s in FSTATS} == {s: d1[s] for s in FSTATS}, (d, d1)
        ix.prof_enable(True)
        ix.flat_knn_mmr(data.qs, 10, 40, 0.5)
        p = ix.prof_get("mmr_select")
        assert p["launches"] == 1 and p["ms"] > 0, p
    finally:
        ix.close()


def test_refused_calls_leave_every_counter(sets):
    import lab_1806_vec_db_amd as vdb

    data = sets["random"]
    base, qs = data.base, data.qs
    ix = _index("l2sqr", base)
    other = _index("l2sqr", base[:100])
    u8 = vdb.GpuIndex(64, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8((base[30:80] * 255).astype(np.uint8))
        mk = ix.make_mask(_allow(len(base), range(100)))
        foreign = other.make_mask(_allow(100, range(10)))
        stale_ix = _index("l2sqr", base[:200])
        stale = stale_ix.make_mask(_allow(200, range(50)))
        stale_ix.batch_add(base[200:210])
        s0, s0_stale, s0_u8 = _stats(ix), _stats(stale_ix), _stats(u8)
        zero = np.zeros(len(qs), dtype=np.uint32)
        bad = [
            (ix, dict(k=10, fetch_k=40, lambda_mult=float("nan")), "lambda"),
            (ix, dict(k=10, fetch_k=40, lambda_mult=-0.5), "lambda"),
            (ix, dict(k=10, fetch_k=40, lambda_mult=1.0001), "lambda"),
            (ix, dict(k=10, fetch_k=9, lambda_mult=0.5), "fetch_k"),
            (ix, dict(k=10, fetch_k=4097, lambda_mult=0.5), "fetch_k"),
            (u8, dict(k=10, fetch_k=40, lambda_mult=0.5), "f32 rows"),
            (ix, dict(k=10, fetch_k=40, lambda_mult=0.5, masks=[mk, foreign], mask_of=zero), None),
            (stale_ix, dict(k=10, fetch_k=40, lambda_mult=0.5, masks=[stale], mask_of=zero), "error 3.*stale"),
            (ix, dict(k=10, fetch_k=40, lambda_mult=0.5, masks=[mk], mask_of=zero + 1), "mask_of"),
        ]
        for index, kw, match in bad:
            with pytest.raises(vdb.VdbError, match=match):
                index.flat_knn_mmr(qs, **kw)
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.flat_knn_mmr(qs[:, :10], 10, 40, 0.5)
        assert _stats(ix) == s0 and _stats(stale_ix) == s0_stale and _stats(u8) == s0_u8
        # empty results: no queries, k = 0, nothing allowed
        gi, gd, gc = ix.flat_knn_mmr(qs[:0], 10, 40, 0.5)
        assert gi.shape[0] == 0 and gc.shape == (0,)
        gi, gd, gc = ix.flat_knn_mmr(qs, 0, 40, 0.5)
        assert (gc == 0).all()
        gi, gd, gc = ix.flat_knn_mmr(qs, 0, 0, 0.5)
        assert (gc == 0).all()
        empty = ix.make_mask(_allow(len(base), []))
        gi, gd, gc = ix.flat_knn_mmr(qs, 10, 40, 0.5, empty)
        assert (gc == 0).all() and (gi == 0).all() and (gd == 0).all()
        for m in (mk, foreign, stale, empty):
            m.close()
        stale_ix.close()
    finally:
        u8.close()
        other.close()
        ix.close()


def test_device_form(sets):
    import torch

    data = sets["random"]
    n, qs = len(data.base), data.qs
    ix = _index("cosine", data.base)
    try:
        ix.set_id_offset(50000)
        nq, k, fk, lam = len(qs), 10, 40, 0.5
        allows = [_allow(n, range(0, n, 2)), _allow(n, range(1, n, 2))]
        masks = [ix.make_mask(a) for a in allows]
        mask_of = (np.arange(nq) % 2).astype(np.uint32)
        tq = torch.from_numpy(qs).cuda()
        for use_masks in (False, True):
            ti = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
            td = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
            tc = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if use_masks:
                ix.flat_knn_mmr_device(tq.data_ptr(), nq, k, fk, lam, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), masks, mask_of)
                exp = data.expect(1, k, fk, lam, allows, mask_of, id_offset=50000)
            else:
                ix.flat_knn_mmr_device(tq.data_ptr(), nq, k, fk, lam, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
                exp = data.expect(1, k, fk, lam, id_offset=50000)
            torch.cuda.synchronize()
            _same((ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().view(np.uint64)), exp, ("device", use_masks))
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_two_threads(sets):
    data = sets["clustered"]
    ix = _index("l2sqr", data.base)
    try:
        args = ((10, 40, 0.5), (5, 64, 0.0))
        exp = {t: data.expect(0, *args[t]) for t in range(2)}
        errs = []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(4):
                    _same(ix.flat_knn_mmr(data.qs, *args[t]), exp[t], ("thread", t))
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        assert ix.get_stat("flat_mmr_calls") == 8 and ix.get_stat("flat_mmr_queries") == 8 * len(data.qs)
    finally:
        ix.close()
