"""GPU: the search by example rows end to end (GpuIndex.flat_knn_like / flat_knn_like_device, vdb_flat_knn_like*).  The reference is the
CPU oracle's full order (oracle.flat_knn at k = n) for the query vector tests/like_ref.py makes from the example rows, restricted in
Python to the allowed rows minus the examples, first k.  Indices and distance bits must match."""
import threading

import numpy as np
import pytest

import like_ref as R

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
LSTATS = ("flat_like_calls", "flat_like_queries", "like_example_rows")
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries", "flat_fallback", "flat_i8_queries", "flat_half_queries",
          "flat_grouped_calls", "flat_grouped_queries", "flat_mmr_calls", "flat_mmr_queries")


def _random_set():
    rng = np.random.default_rng(6101)
    base = rng.random((2000, 64)).astype(np.float32)
    base[5, 17] = np.nan     # NaN distance to every query: last in every order (never an example here)
    base[20:30] = base[3]    # identical rows: equal distances, ordered by id
    pick = lambda m: rng.choice(np.arange(40, 2000), m, replace=False).tolist()
    pos = [[77], pick(5), pick(3), pick(50), [3, 21], [7, 7, 9], [100], [1999, 0]]
    neg = [[], [], pick(2), pick(5), [20, 22], [9], [101], []]
    return base, pos, neg


def _clustered_set():
    """20 clusters of 8 near-duplicates each (row r belongs to cluster r % 20): "more like these" with examples from one cluster finds
    the rest of that cluster first -- and with exclusion off, the examples themselves"""
    rng = np.random.default_rng(6102)
    centres = rng.random((20, 64)).astype(np.float32)
    base = (centres[np.arange(160) % 20] + rng.standard_normal((160, 64)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    pos = [[0], [1, 21, 41], [2, 22], [3, 23, 43, 63, 83, 103, 123, 143], [4], [5, 25, 5], [6, 7], [19, 39]]
    neg = [[], [], [3, 23], [4], [24, 44, 64], [], [8, 28], [19]]
    return base, pos, neg


class Data:
    def __init__(self, base, pos, neg):
        from oracle import oracle as O

        self.base, self.pos, self.neg = base, pos, neg
        self.n, self.nq = len(base), len(pos)
        self.qs = R.like_queries(base, pos, neg)
        self.full = {}
        for _, kind in DISTS:  # computed once, shared, never changed
            oi, od, oc = O.flat_knn_batch(base, self.qs, len(base), kind, nthreads=16)
            assert (oc == len(base)).all()
            self.full[kind] = (oi.astype(np.int64), od)

    def expect(self, kind, k, exclude=True, allows=None, mask_of=None, id_offset=0, full=None, pos=None, neg=None):
        oi, od = full if full is not None else self.full[kind]
        pos, neg = pos or self.pos, neg or self.neg
        kk = max(k, 1)
        idx = np.zeros((len(oi), kk), dtype=np.uint64)
        dist = np.zeros((len(oi), kk), dtype=np.float32)
        cnt = np.zeros(len(oi), dtype=np.uint64)
        for q in range(len(oi)):
            rows, d = oi[q], od[q]
            keep = np.ones(len(rows), dtype=np.bool_)
            if allows is not None:
                keep &= allows[int(mask_of[q])][rows]
            if exclude:
                keep &= ~np.isin(rows, np.asarray(list(pos[q]) + list(neg[q]), dtype=np.int64))
            rows, d = rows[keep][:k], d[keep][:k]
            cnt[q] = len(rows)
            idx[q, :len(rows)] = rows.astype(np.uint64) + np.uint64(id_offset)
            dist[q, :len(rows)] = d
        return idx[:, :k], dist[:, :k], cnt


@pytest.fixture(scope="module")
def sets():
    return {"random": Data(*_random_set()), "clustered": Data(*_clustered_set())}


def _same(got, exp, what=""):
    gi, gd, gc = got
    ei, ed, ec = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), (what, gi[:2], ei[:2])
    assert gd.dtype == np.float32 and np.array_equal(np.isnan(gd), np.isnan(ed)), what  # (a NaN's payload is not part of the search's contract)
    ok = ~np.isnan(ed)
    assert np.array_equal(gd[ok].view(np.uint32), ed[ok].view(np.uint32)), what


def _stats(ix, names=LSTATS + FSTATS):
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


def _plain_device(ix, qs, k):
    """vdb_flat_knn_device: the call the unfiltered search by example makes for its lists"""
    import torch

    nq = len(qs)
    tq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    ti = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    td = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    tc = torch.zeros((nq,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.flat_knn_device(tq.data_ptr(), nq, k, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
    torch.cuda.synchronize()


def test_the_reference_leaves_examples_out_and_finds_the_cluster(sets):
    """on the CPU, before anything runs on the GPU: the reference differs from the plain top k of its own query (so no test below can
    pass by returning the plain k-NN), and on the clustered set the answers are what the feature is for"""
    data = sets["clustered"]
    ei, _, ec = data.expect(0, 5)
    plain = data.full[0][0][:, :5]
    assert (ec == 5).all() and all(ei[q].tolist() != plain[q].tolist() for q in range(data.nq))
    assert set((ei[0] % 20).tolist()) == {0} and 0 not in ei[0].tolist()   # the rest of row 0's cluster
    assert data.expect(0, 1, exclude=False)[0][0, 0] == 0                  # one positive, exclusion off: hit 0 is the row itself


@pytest.mark.parametrize("name", ("random", "clustered"))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_cases_against_the_oracle(sets, name, dist, kind):
    from oracle import oracle as O

    data = sets[name]
    ix = _index(dist, data.base)
    try:
        for k in (1, 10, 64, 100):
            for exclude in (True, False):
                s0 = _stats(ix, LSTATS)
                got = ix.flat_knn_like(data.pos, k, data.neg, exclude)
                d = _delta(ix, s0)
                _same(got, data.expect(kind, k, exclude), (name, dist, k, exclude))
                assert d == {"flat_like_calls": 1, "flat_like_queries": data.nq, "like_example_rows": sum(map(len, data.pos)) + sum(map(len, data.neg))}, d
        gi, gd, gc = ix.flat_knn_like(data.pos, 3, data.neg, exclude=False)
        assert gi[0, 0] == data.pos[0][0] and gc[0] == 3  # one positive, exclusion off: hit 0 is the row itself
        # k past the table: every row that is no example, the NaN row of the random set last
        k = data.n + 5
        got = ix.flat_knn_like(data.pos, k, data.neg)
        _same(got, data.expect(kind, k), (name, dist, "every row"))
        assert got[2][3] == data.n - len(set(data.pos[3]) | set(data.neg[3]))
        _same(ix.flat_knn_like(data.pos, k, data.neg, exclude=False), data.expect(kind, k, False), (name, dist, "every row, examples kept"))
        # no negatives at all (neg_lims == NULL)
        qs = R.like_queries(data.base, data.pos)
        oi, od, _ = O.flat_knn_batch(data.base, qs, data.n, kind, nthreads=16)
        none = [[] for _ in data.pos]
        _same(ix.flat_knn_like(data.pos, 10), data.expect(kind, 10, full=(oi.astype(np.int64), od), neg=none), (name, dist, "positives only"))
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_with_masks_on_both_routes(sets, dist, kind):
    """one mask for every query, and a mask per query -- an empty one (m = 0), one shorter than k (m < k), one that holds fewer than k
    rows besides the examples (m - examples < k), examples outside the query's mask, long ones -- with the masks of up to
    "flat_filtered_direct_max" rows in the filtered call's one launch and the longer ones on its per-mask route"""
    data = sets["random"]
    n, nq = data.n, data.nq
    rng = np.random.default_rng(8)
    ex3 = data.pos[3] + data.neg[3]
    allows = [_allow(n, rng.choice(n, 1200, replace=False)), _allow(n, []), _allow(n, rng.choice(n, 5, replace=False)),
              _allow(n, ex3[:50] + list(range(40, 46))), np.ones(n, dtype=np.bool_), _allow(n, np.arange(2, n, 3))]
    ix = _index(dist, data.base)
    try:
        masks = [ix.make_mask(a) for a in allows]
        zero = np.zeros(nq, dtype=np.uint32)
        mask_of = np.array([0, 1, 2, 3, 4, 5, 5, 0], dtype=np.uint32)
        assert not allows[5][data.pos[6][0]] and not allows[5][data.pos[5][1]]  # examples outside the query's mask: nothing to leave out
        for direct_max in (8192, 100):  # 100: the masks of 1200, 2000 and 666 rows leave the one launch
            ix.set_param("flat_filtered_direct_max", direct_max)
            for k, exclude in ((10, True), (10, False), (3, True)):
                s0 = _stats(ix)
                got = ix.flat_knn_like(data.pos, k, data.neg, exclude, masks[0])
                d = _delta(ix, s0)
                _same(got, data.expect(kind, k, exclude, allows[:1], zero), (dist, direct_max, k, exclude, "one mask"))
                # the underlying search's counters advance as for vdb_flat_knn_filtered_multi at k = the list length K'
                kp = k + max(len(p) + len(g) for p, g in zip(data.pos, data.neg)) if exclude else k
                s1 = _stats(ix)
                ix.flat_knn_filtered_multi(data.qs, kp, masks[:1], zero)
                d1 = _delta(ix, s1)
                assert d["flat_like_calls"] == 1 and d["flat_like_queries"] == nq and d1["flat_like_calls"] == 0
                assert {s: d[s] for s in FSTATS} == {s: d1[s] for s in FSTATS}, (d, d1)
                got = ix.flat_knn_like(data.pos, k, data.neg, exclude, masks, mask_of)
                _same(got, data.expect(kind, k, exclude, allows, mask_of), (dist, direct_max, k, exclude, "mask per query"))
                assert got[2][1] == 0 and got[2][2] == min(k, 5)
                if exclude:
                    assert got[2][3] == min(k, int(allows[3].sum()) - len(set(ex3) & set(np.flatnonzero(allows[3]).tolist())))
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_list_length_64_and_65_and_the_counters_of_the_search_under_it(sets):
    """k + e_max = 64 is the last list on the 8-bit first pass of the searches, 65 the first past it; the counters of the search under the
    call are those of a plain vdb_flat_knn_device at K'"""
    from oracle import oracle as O

    data = sets["random"]
    ix = _index("l2sqr", data.base)
    try:
        pos = [list(range(100, 150)), [300]]
        for n_neg, kp in ((4, 64), (5, 65)):
            neg = [list(range(200, 200 + n_neg)), []]
            qs = R.like_queries(data.base, pos, neg)
            oi, od, _ = O.flat_knn_batch(data.base, qs, data.n, 0, nthreads=16)
            for exclude in (True, False):
                s0 = _stats(ix)
                got = ix.flat_knn_like(pos, 10, neg, exclude)
                d = _delta(ix, s0)
                _same(got, data.expect(0, 10, exclude, full=(oi.astype(np.int64), od), pos=pos, neg=neg), (kp, exclude))
                s1 = _stats(ix)
                _plain_device(ix, qs, kp if exclude else 10)
                d1 = _delta(ix, s1)
                assert d["flat_like_calls"] == 1 and d["flat_like_queries"] == 2 and d["like_example_rows"] == 51 + n_neg
                assert {s: d[s] for s in FSTATS} == {s: d1[s] for s in FSTATS}, (d, d1)
        ix.prof_enable(True)
        ix.flat_knn_like(pos, 10, neg)
        for name in ("like_build", "like_drop"):
            p = ix.prof_get(name)
            assert p["launches"] == 1 and p["ms"] > 0, (name, p)
    finally:
        ix.close()


def test_refused_calls_leave_every_counter(sets):
    import lab_1806_vec_db_amd as vdb

    data = sets["random"]
    base, nq = data.base, data.nq
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
        zero = np.zeros(nq, dtype=np.uint32)
        small = [[p[0] % 50] for p in data.pos]
        bad = [
            (ix, dict(positives=[[1]] * 7 + [[]], k=10), "at least one positive"),
            (ix, dict(positives=[[1]] * 7 + [list(range(1025))], k=10), "at most 1024"),
            (ix, dict(positives=[[1]] * 8, k=10, negatives=[[]] * 7 + [list(range(1024))]), "at most 1024"),
            (ix, dict(positives=[[1]] * 7 + [[2000]], k=10), "no row of this index"),
            (ix, dict(positives=[[1]] * 8, k=10, negatives=[[]] * 7 + [[1 << 35]]), "no row of this index"),
            (u8, dict(positives=small, k=10), "f32 rows"),
            (ix, dict(positives=data.pos, k=10, masks=[mk, foreign], mask_of=zero), None),
            (stale_ix, dict(positives=small, k=10, masks=[stale], mask_of=zero), "error 3.*stale"),
            (ix, dict(positives=data.pos, k=10, masks=[mk], mask_of=zero + 1), "mask_of"),
        ]
        for index, kw, match in bad:
            with pytest.raises(vdb.VdbError, match=match):
                index.flat_knn_like(**kw)
        assert _stats(ix) == s0 and _stats(stale_ix) == s0_stale and _stats(u8) == s0_u8
        # empty results: no queries, k = 0, nothing allowed
        gi, gd, gc = ix.flat_knn_like([], 10)
        assert gi.shape[0] == 0 and gc.shape == (0,)
        gi, gd, gc = ix.flat_knn_like(data.pos, 0, data.neg)
        assert (gc == 0).all()
        empty = ix.make_mask(_allow(len(base), []))
        gi, gd, gc = ix.flat_knn_like(data.pos, 10, data.neg, True, empty)
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

    import lab_1806_vec_db_amd as vdb

    data = sets["random"]
    n, nq, k, off = data.n, data.nq, 10, 50000
    ix = _index("cosine", data.base)
    try:
        ix.set_id_offset(off)
        allows = [_allow(n, range(0, n, 2)), _allow(n, range(1, n, 2))]
        masks = [ix.make_mask(a) for a in allows]
        mask_of = (np.arange(nq) % 2).astype(np.uint32)
        lims = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.uint64)
        flat = lambda ls, o=off: torch.from_numpy(np.asarray([r + o for x in ls for r in x], dtype=np.int64)).cuda()
        t_p, t_n = flat(data.pos), flat(data.neg)

        def run(use_masks, exclude, tp=t_p):
            ti = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
            td = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
            tc = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            try:
                ix.flat_knn_like_device(lims(data.pos), tp.data_ptr(), lims(data.neg), t_n.data_ptr(), nq, k, ti.data_ptr(), td.data_ptr(), tc.data_ptr(),
                                        exclude, masks if use_masks else None, mask_of if use_masks else None)
            finally:
                torch.cuda.synchronize()
                run.last = (ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().view(np.uint64))
            return run.last

        for use_masks in (False, True):
            for exclude in (True, False):
                exp = data.expect(1, k, exclude, allows if use_masks else None, mask_of if use_masks else None, id_offset=off)
                _same(run(use_masks, exclude), exp, ("device", use_masks, exclude))
        # an id that is no row of the index (a LOCAL id under an id_offset): refused, outputs and counters untouched
        s0 = _stats(ix)
        with pytest.raises(vdb.VdbError, match="no row of this index"):
            run(False, True, flat(data.pos, 0))
        assert all((a.view(np.int64) == -1).all() for a in (run.last[0], run.last[2])) and (run.last[1] == -1.0).all()
        assert _stats(ix) == s0
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_two_threads(sets):
    data = sets["clustered"]
    ix = _index("l2sqr", data.base)
    try:
        args = ((10, True), (5, False))
        exp = {t: data.expect(0, *args[t]) for t in range(2)}
        errs = []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(4):
                    _same(ix.flat_knn_like(data.pos, args[t][0], data.neg, args[t][1]), exp[t], ("thread", t))
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        assert ix.get_stat("flat_like_calls") == 8 and ix.get_stat("flat_like_queries") == 8 * data.nq
    finally:
        ix.close()
