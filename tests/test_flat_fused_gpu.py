"""GPU: the fused multi-query search end to end (GpuIndex.flat_knn_fused / flat_knn_fused_device, vdb_flat_knn_fused*).  The reference is
the CPU oracle's full order (oracle.flat_knn at k = n) of every sub-query, restricted in Python to the sub-query's allowed rows, cut at
fetch_k and pushed through tests/fuse_ref.py; MIN additionally against the oracle's min-over-sub-queries order computed without any
lists.  Ids, order, score bits, counts and the zeros behind the counts must match."""
import threading

import numpy as np
import pytest

import fuse_ref as R

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
USTATS = ("flat_fused_calls", "flat_fused_queries", "flat_fused_lists")
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries", "flat_fallback", "flat_i8_queries", "flat_half_queries",
          "flat_grouped_calls", "flat_grouped_queries", "flat_mmr_calls", "flat_mmr_queries", "flat_like_calls", "flat_like_queries")
SIZES = (1, 2, 3, 4, 8, 1, 5)  # sub-queries of the fused queries: ragged
N, DIM = 3000, 20


def _random_set():
    rng = np.random.default_rng(7101)
    base = rng.random((N, DIM)).astype(np.float32)
    base[20:30] = base[3]  # identical rows: equal distances, ordered by id
    qs = rng.random((sum(SIZES), DIM)).astype(np.float32)
    qs[1] = base[3]        # a sub-query that is a stored row: distance 0 to eleven rows
    qs[4] = qs[3]          # two sub-queries of one fused query with the same vector: full overlap
    return base, qs


def _clustered_set():
    """20 clusters of 150 near-duplicates each (row r belongs to cluster r % 20); the sub-queries of a fused query sit in neighbouring
    clusters, some in the same one: lists that overlap in part, in full and not at all"""
    rng = np.random.default_rng(7102)
    centres = rng.random((20, DIM)).astype(np.float32)
    base = (centres[np.arange(N) % 20] + rng.standard_normal((N, DIM)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    cl = [0, 1, 1, 2, 3, 3, 4, 5, 6, 7, 8, 8, 9, 9, 10, 11, 12, 13, 14, 14, 15, 16, 17, 18]
    qs = (centres[cl] + rng.standard_normal((len(cl), DIM)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    return base, qs


class Data:
    def __init__(self, base, qs):
        from oracle import oracle as O

        self.base, self.qs = base, qs
        self.lims = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
        self.full = {}
        for _, kind in DISTS:  # computed once, shared, never changed
            oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
            assert (oc == len(base)).all() and not np.isnan(od).any()
            self.full[kind] = (oi.astype(np.int64), od)

    def lists(self, kind, q, fetch_k, allows=None, mask_of=None, lims=None):
        lims = self.lims if lims is None else lims
        oi, od = self.full[kind]
        out = []
        for j in range(int(lims[q]), int(lims[q + 1])):
            rows, d = oi[j], od[j]
            if allows is not None:
                keep = allows[int(mask_of[j])][rows]
                rows, d = rows[keep], d[keep]
            out.append((rows[:fetch_k], d[:fetch_k]))
        return out

    def expect(self, kind, k, fetch_k, mode, weights=None, c=60.0, allows=None, mask_of=None, id_offset=0, lims=None):
        lims = self.lims if lims is None else lims
        nq, kk = len(lims) - 1, max(k, 1)
        idx, bits, cnt = np.zeros((nq, kk), np.uint64), np.zeros((nq, kk), np.uint32), np.zeros(nq, np.uint64)
        for q in range(nq):
            w = None if weights is None else weights[int(lims[q]):int(lims[q + 1])]
            ids, sc = R.fuse(self.lists(kind, q, fetch_k, allows, mask_of, lims), k, mode, w, c)
            idx[q], bits[q], cnt[q] = R.padded(ids + np.uint64(id_offset), sc, kk)
        return idx[:, :k], bits[:, :k], cnt

    def min_direct(self, kind, q, k, allows=None, mask_of=None):
        """the k allowed rows nearest to any sub-query of fused query q, from the full distance table: no lists, no fetch_k"""
        oi, od = self.full[kind]
        n = len(self.base)
        js = range(int(self.lims[q]), int(self.lims[q + 1]))
        d_of = np.empty((len(js), n), dtype=np.float32)
        keys = np.full((len(js), n), 1 << 32, dtype=np.int64)  # (past every key: the row is not allowed to this sub-query)
        for s, j in enumerate(js):
            d_of[s, oi[j]] = od[j]
            u = (d_of[s] + np.float32(0.0)).view(np.uint32).astype(np.int64)  # f32_orderable, no NaN here
            o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
            ok = np.ones(n, dtype=np.bool_) if allows is None else allows[int(mask_of[j])]
            keys[s, ok] = o[ok]
        first = keys.argmin(axis=0)  # the first sub-query that attains the minimum
        best = keys[first, np.arange(n)]
        rows = np.flatnonzero(best < (1 << 32))
        rows = rows[np.lexsort((rows, best[rows]))][:k]
        return rows.tolist(), d_of[first[rows], rows].view(np.uint32).tolist()


@pytest.fixture(scope="module")
def sets():
    return {"random": Data(*_random_set()), "clustered": Data(*_clustered_set())}


def _same(got, exp, what=""):
    gi, gd, gc = got
    ei, eb, ec = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), (what, gi[:2], ei[:2])
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), eb), (what, gd[:2], eb.view(np.float32)[:2])


def _stats(ix, names=USTATS + FSTATS):
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


def _device(ix, qs, lims, k, fetch_k, **kw):
    import torch

    nq, kk = len(lims) - 1, max(k, 1)
    tq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    ti = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    td = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    tc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.flat_knn_fused_device(tq.data_ptr(), lims, k, fetch_k, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), **kw)
    finally:
        torch.cuda.synchronize()
        _device.last = (ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().view(np.uint64))
    return _device.last


@pytest.mark.parametrize("name", ("random", "clustered"))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_cases_against_the_oracle(sets, name, dist, kind):
    D = sets[name]
    ix = _index(dist, D.base)
    try:
        w = np.random.default_rng(5).uniform(0.25, 4.0, size=len(D.qs)).astype(np.float32)
        for k, fetch_k in ((10, 10), (10, 40), (10, 64), (10, 65), (1, 1), (100, 300), (0, 5)):
            for mode, weights, c in (("rrf", None, 60.0), ("rrf", w, 0.0), ("min", None, 60.0)):
                got = ix.flat_knn_fused(D.qs, D.lims, k, fetch_k, mode, weights, c)
                _same(got, D.expect(kind, k, fetch_k, mode, weights, c), f"{name} {dist} k={k} F={fetch_k} {mode}")
        # MIN with fetch_k >= k is the k rows nearest to ANY of the sub-queries over the whole table
        for k, fetch_k in ((10, 10), (10, 64), (50, 50)):
            gi, gd, gc = ix.flat_knn_fused(D.qs, D.lims, k, fetch_k, "min")
            for q in range(len(SIZES)):
                rows, bits = D.min_direct(kind, q, k)
                assert gc[q] == k and gi[q].tolist() == rows and gd[q].view(np.uint32).tolist() == bits, (name, dist, k, fetch_k, q)
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_one_sub_query_is_the_plain_search(sets, dist, kind):
    D = sets["random"]
    ix = _index(dist, D.base)
    try:
        nsub = len(D.qs)
        lims = np.arange(nsub + 1, dtype=np.uint64)
        for k in (1, 10, 64, 65):
            pi, pd, pc = ix.flat_knn(D.qs, k)
            mi, md, mc = ix.flat_knn_fused(D.qs, lims, k, k, "min")
            assert np.array_equal(mi, pi) and np.array_equal(md.view(np.uint32), pd.view(np.uint32)) and np.array_equal(mc, pc), k
            ri, rd, rc = ix.flat_knn_fused(D.qs, lims, k, k, "rrf")
            assert np.array_equal(ri, pi) and np.array_equal(rc, pc) and (np.diff(rd, axis=1) < 0).all(), k
        allows = [_allow(N, np.arange(0, N, 3)), _allow(N, np.arange(100, 140))]
        masks = [ix.make_mask(a) for a in allows]
        mo = (np.arange(nsub) % 2).astype(np.uint32)
        pi, pd, pc = ix.flat_knn_filtered_multi(D.qs, 50, masks, mo)
        mi, md, mc = ix.flat_knn_fused(D.qs, lims, 50, 50, "min", masks=masks, mask_of=mo)
        assert np.array_equal(mi, pi) and np.array_equal(md.view(np.uint32), pd.view(np.uint32)) and np.array_equal(mc, pc)
        assert sorted(set(mc.tolist())) == [40, 50]
    finally:
        ix.close()


@pytest.mark.parametrize("direct_max", (8192, 500))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_with_masks_on_both_routes(sets, dist, kind, direct_max):
    """masks up to flat_filtered_direct_max rows share the grouped launch, longer ones take the per-mask route"""
    D = sets["clustered"]
    ix = _index(dist, D.base)
    try:
        ix.set_param("flat_filtered_direct_max", direct_max)
        nsub = len(D.qs)
        allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400)), _allow(N, [7, 27, 47, 1007, 2999]), _allow(N, []),
                  _allow(N, np.arange(N))]
        masks = [ix.make_mask(a) for a in allows]
        one = np.zeros(nsub, dtype=np.uint32)
        per = (np.arange(nsub) % 5).astype(np.uint32)   # every fused query of 3 or more sees a short mask; some sub-queries see none at all
        none = np.full(nsub, 3, dtype=np.uint32)
        for mo, what in ((one, "one mask"), (per, "a mask per sub-query"), (none, "nothing allowed")):
            for k, fetch_k in ((10, 10), (10, 64), (10, 65), (5, 300)):
                for mode in ("rrf", "min"):
                    got = ix.flat_knn_fused(D.qs, D.lims, k, fetch_k, mode, masks=masks, mask_of=mo)
                    _same(got, D.expect(kind, k, fetch_k, mode, allows=allows, mask_of=mo), f"{dist} {what} k={k} F={fetch_k} {mode}")
        gi, gd, gc = ix.flat_knn_fused(D.qs, D.lims, 10, 64, "min", masks=masks, mask_of=per)
        for q in range(len(SIZES)):
            rows, bits = D.min_direct(kind, q, 10, allows, per)
            assert gi[q, :int(gc[q])].tolist() == rows and gd[q, :int(gc[q])].view(np.uint32).tolist() == bits, q
        got = ix.flat_knn_fused(D.qs, D.lims, 10, 64, "rrf", masks=masks[1], mask_of=None)  # one RowMask for every sub-query
        _same(got, D.expect(kind, 10, 64, "rrf", allows=allows, mask_of=np.ones(nsub, dtype=np.uint32)), "single mask")
        assert (ix.flat_knn_fused(D.qs, D.lims, 10, 64, "rrf", masks=masks, mask_of=none)[2] == 0).all()
    finally:
        ix.close()


def test_counters_of_the_call_and_of_the_searches_under_it(sets):
    import torch

    D = sets["random"]
    nsub, nq = len(D.qs), len(SIZES)
    a, b = _index("l2sqr", D.base), _index("l2sqr", D.base)
    try:
        for fetch_k in (64, 65):
            # unfiltered: the counters of ONE vdb_flat_knn_device call over the sub-queries at K' = fetch_k
            tq = torch.from_numpy(D.qs).cuda()
            ti = torch.zeros((nsub, fetch_k), dtype=torch.int64, device="cuda")
            td = torch.zeros((nsub, fetch_k), dtype=torch.float32, device="cuda")
            tc = torch.zeros((nsub,), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            s0 = _stats(b)
            b.flat_knn_device(tq.data_ptr(), nsub, fetch_k, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
            under = _delta(b, s0)
            s0 = _stats(a)
            a.flat_knn_fused(D.qs, D.lims, 10, fetch_k, "rrf")
            assert _delta(a, s0) == {**under, "flat_fused_calls": 1, "flat_fused_queries": nq, "flat_fused_lists": nsub}, fetch_k
            # filtered: ONE vdb_flat_knn_filtered_multi call
            allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400))]
            mo = (np.arange(nsub) % 2).astype(np.uint32)
            s0 = _stats(b)
            b.flat_knn_filtered_multi(D.qs, fetch_k, [b.make_mask(x) for x in allows], mo)
            under = _delta(b, s0)
            assert under["flat_filtered_multi_calls"] == 1
            s0 = _stats(a)
            a.flat_knn_fused(D.qs, D.lims, 10, fetch_k, "min", masks=[a.make_mask(x) for x in allows], mask_of=mo)
            assert _delta(a, s0) == {**under, "flat_fused_calls": 1, "flat_fused_queries": nq, "flat_fused_lists": nsub}, fetch_k
        s0 = _stats(a)
        a.flat_knn_fused(D.qs[:0], [0], 10, 40)  # no fused query: a call all the same, nothing else
        a.flat_knn_fused(D.qs, D.lims, 0, 40)    # k == 0: counted, no search under it
        assert _delta(a, s0) == {**{s: 0 for s in FSTATS}, "flat_fused_calls": 2, "flat_fused_queries": nq, "flat_fused_lists": nsub}
        a.prof_enable(True)
        a.prof_reset()
        a.flat_knn_fused(D.qs, D.lims, 10, 40)
        p = a.prof_get("fuse_lists")
        assert p["launches"] == 1 and p["ms"] > 0, p
    finally:
        a.close()
        b.close()


def test_device_form_and_id_offset(sets):
    D = sets["clustered"]
    ix = _index("cosine", D.base)
    try:
        w = np.linspace(0.5, 2.0, len(D.qs)).astype(np.float32)
        allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400))]
        masks = [ix.make_mask(x) for x in allows]
        mo = (np.arange(len(D.qs)) % 2).astype(np.uint32)
        for off in (0, (1 << 33) + 3):
            ix.set_id_offset(off)
            _same(_device(ix, D.qs, D.lims, 10, 40, mode="rrf", weights=w, rrf_c=1.0), D.expect(1, 10, 40, "rrf", w, 1.0, id_offset=off), "device rrf")
            _same(_device(ix, D.qs, D.lims, 80, 80, mode="min"), D.expect(1, 80, 80, "min", id_offset=off), "device min")
            _same(_device(ix, D.qs, D.lims, 10, 65, mode="min", masks=masks, mask_of=mo),
                  D.expect(1, 10, 65, "min", allows=allows, mask_of=mo, id_offset=off), "device masks")
            _same(ix.flat_knn_fused(D.qs, D.lims, 10, 40, "rrf", w, 1.0), D.expect(1, 10, 40, "rrf", w, 1.0, id_offset=off), "host form")
        ix.set_id_offset(0)
        gi, gd, gc = _device(ix, D.qs, D.lims, 0, 0)  # k == 0: counts only, no slot touched
        assert (gc == 0).all() and (gi == np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)).all()
    finally:
        ix.close()


def test_refused_calls_leave_every_counter(sets):
    import lab_1806_vec_db_amd as vdb

    D = sets["random"]
    ix = _index("l2sqr", D.base)
    other = _index("l2sqr", D.base[:100])
    try:
        mk, foreign = ix.make_mask(np.arange(50)), other.make_mask(np.arange(50))
        nsub = len(D.qs)
        s0 = _stats(ix)
        sent = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)

        def refused(match, *a, exc=vdb.VdbError, lims=D.lims, qs=D.qs, **kw):
            with pytest.raises(exc, match=match):
                _device(ix, qs, lims, *a, **kw)
            gi, gd, gc = _device.last
            assert (gi == sent).all() and (gd == -7.0).all() and (gc == sent).all(), match
            with pytest.raises(exc, match=match):
                ix.flat_knn_fused(qs, lims, *a, **kw)

        refused("mode", 10, 40, mode=5)
        refused("start at 0", 10, 40, lims=D.lims + np.uint64(1), qs=np.concatenate([D.qs, D.qs[:1]]))
        bad = D.lims.copy()
        bad[2], bad[3] = bad[3], bad[2]
        refused("not decrease", 10, 40, lims=bad)
        refused("at least one sub-query", 10, 40, lims=np.concatenate([D.lims[:3], D.lims[2:]]))
        refused("at most 32", 10, 40, lims=np.array([0, 33], dtype=np.uint64), qs=np.zeros((33, DIM), np.float32))
        refused("at least k", 41, 40)
        refused("at most 4096", 10, 4097)
        refused("at most 16384", 10, 4096)  # 8 sub-queries x 4096
        refused("weight", 10, 40, weights=np.r_[np.ones(nsub - 1), 0.0])
        refused("weight", 10, 40, weights=np.r_[np.nan, np.ones(nsub - 1)])
        refused("weight", 10, 40, weights=np.r_[np.inf, np.ones(nsub - 1)])
        refused("VDB_FUSE_RRF only", 10, 40, mode="min", weights=np.ones(nsub))
        for c in (-1.0, float("nan"), float("inf")):
            refused("rrf_c", 10, 40, rrf_c=c)
        refused("mask_of", 10, 40, masks=[mk], mask_of=np.full(nsub, 1, dtype=np.uint32))
        refused("mask", 10, 40, masks=[foreign], mask_of=np.zeros(nsub, dtype=np.uint32))
        assert _delta(ix, s0) == {s: 0 for s in s0}
        ix.batch_add(D.base[:1])  # the mask is stale now
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_fused(D.qs, D.lims, 10, 40, masks=[mk], mask_of=np.zeros(nsub, dtype=np.uint32))
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.flat_knn_fused(np.zeros((nsub, DIM + 1), np.float32), D.lims, 10, 40)
        assert _delta(ix, s0) == {s: 0 for s in s0}
        u8 = vdb.GpuIndex(DIM, "l2sqr", scalar="u8")
        try:
            u8.batch_add_u8(np.zeros((8, DIM), dtype=np.uint8))
            with pytest.raises(vdb.VdbError, match="f32 rows"):
                u8.flat_knn_fused(D.qs, D.lims, 10, 40)
            assert u8.get_stat("flat_fused_calls") == 0
        finally:
            u8.close()
    finally:
        ix.close()
        other.close()


def test_more_sub_queries_than_one_list_call_takes(sets):
    """9000 fused queries of 2 sub-queries: the host form cuts them into chunks of whole fused queries (16384 sub-queries at most), the
    device form takes all 18000 and the driver cuts them itself; the lists are flat_knn's (held against the oracle above)"""
    D = sets["random"]
    ix = _index("l2sqr", D.base)
    try:
        nq, S, k, fk = 9000, 2, 3, 4
        qs = np.random.default_rng(17).random((nq * S, DIM)).astype(np.float32)
        lims = np.arange(0, nq * S + 1, S, dtype=np.uint64)
        w = np.tile(np.array([1.0, 0.5], dtype=np.float32), nq)
        li, ld, lc = ix.flat_knn(qs, fk)
        assert (lc == fk).all()
        for mode, weights in (("rrf", w), ("min", None)):
            ei, eb = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.uint32)
            for q in range(nq):
                ids, sc = R.fuse([(li[j], ld[j]) for j in (2 * q, 2 * q + 1)], k, mode, None if weights is None else weights[2 * q:2 * q + 2])
                ei[q], eb[q], c = R.padded(ids, sc, k)
                assert c == k
            exp = (ei, eb, np.full(nq, k, dtype=np.uint64))
            _same(ix.flat_knn_fused(qs, lims, k, fk, mode, weights), exp, f"host chunks {mode}")
            _same(_device(ix, qs, lims, k, fk, mode=mode, weights=weights), exp, f"device sub-chunks {mode}")
    finally:
        ix.close()


def test_two_threads(sets):
    D = sets["clustered"]
    ix = _index("l2sqr", D.base)
    try:
        jobs = (("rrf", 40), ("min", 65))
        exp = [D.expect(0, 10, f, m) for m, f in jobs]
        err = []

        def work(t):
            try:
                for _ in range(6):
                    _same(ix.flat_knn_fused(D.qs, D.lims, 10, jobs[t][1], jobs[t][0]), exp[t], f"thread {t}")
            except Exception as e:  # noqa: BLE001
                err.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not err, err
    finally:
        ix.close()
