"""GPU: the document-level fused search end to end (GpuIndex.flat_knn_fused_groups / flat_knn_fused_groups_device,
vdb_flat_knn_fused_groups*) on 3000 x 24 with labels row // 7, about 5 % of the rows unlabelled, NaN rows and duplicate rows.  The
reference is the CPU oracle's full order (oracle.flat_knn at k = n) of every sub-query, restricted in Python to the sub-query's allowed
rows, cut at fetch_k and pushed through tests/fuse_groups_ref.py; at fetch_k = n additionally against sums and minima taken straight from
the oracle's distance table, without lists.  Representatives, order, score bits, counts, the zeros behind the counts and `exact` must
match.  (The payload of a NaN DISTANCE is not part of the search's contract: NaN scores are compared as NaN.)"""
import numpy as np
import pytest

import fuse_groups_ref as R
import fuse_ref

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
MODES = ("rrf", "min", "sum")
USTATS = ("flat_fused_groups_calls", "flat_fused_groups_queries", "flat_fused_groups_lists")
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries", "flat_fallback", "flat_i8_queries", "flat_half_queries",
          "flat_grouped_calls", "flat_grouped_queries", "flat_fused_calls", "flat_fused_queries", "flat_fused_lists")
SIZES = (1, 2, 3, 4, 8, 1, 5)   # sub-queries of the fused queries: ragged
SIZES_FULL = (1, 2, 3, 4, 5)    # ... of the calls at fetch_k = n (sub-queries x fetch_k <= 16384)
N, DIM, COL = 3000, 24, 3
NONE = 0xFFFFFFFF
SENT = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)


def _labels():
    rng = np.random.default_rng(7200)
    lab = (np.arange(N) // 7).astype(np.uint32)
    lab[rng.random(N) < 0.05] = NONE
    lab[5], lab[77] = 0, NONE  # the NaN rows: one inside document 0, one a group of its own
    return lab


def _random_set():
    rng = np.random.default_rng(7201)
    base = rng.random((N, DIM)).astype(np.float32)
    base[20:30] = base[3]  # identical rows: equal distances, ordered by id
    base[5, 17] = np.nan   # NaN distance to every query: last in every order
    base[77, 3] = np.nan
    qs = rng.random((sum(SIZES), DIM)).astype(np.float32)
    qs[1] = base[3]        # a sub-query that is a stored row
    qs[4] = qs[3]          # two sub-queries of one fused query with the same vector
    return base, qs


def _clustered_set():
    """20 clusters; the 7 rows of a document (row // 7) lie in one cluster, (row // 7) % 20, as near-duplicates: the nearest ROWS of a query
    are several chunks of few documents; the sub-queries of a fused query sit in neighbouring clusters, some in the same one"""
    rng = np.random.default_rng(7202)
    centres = rng.random((20, DIM)).astype(np.float32)
    base = (centres[(np.arange(N) // 7) % 20] + rng.standard_normal((N, DIM)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    cl = [0, 1, 1, 2, 3, 3, 4, 5, 6, 7, 8, 8, 9, 9, 10, 11, 12, 13, 14, 14, 15, 16, 17, 18]
    qs = (centres[cl] + rng.standard_normal((len(cl), DIM)).astype(np.float32) * np.float32(0.002)).astype(np.float32)
    return base, qs


def _lims(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def _canon(bits):
    b = np.array(bits, dtype=np.uint32)
    b[(b & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
    return b


class Data:
    def __init__(self, base, qs):
        from oracle import oracle as O

        self.base, self.qs, self.labels = base, qs, _labels()
        self.lims = _lims(SIZES)
        self.group_of = R.label_groups(self.labels)
        self.full = {}
        for _, kind in DISTS:  # computed once, shared, never changed
            oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
            assert (oc == len(base)).all()
            self.full[kind] = (oi.astype(np.int64), od)

    def lists(self, kind, q, fetch_k, lims, allows=None, mask_of=None):
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
        idx, bits, cnt, exact = np.zeros((nq, kk), np.uint64), np.zeros((nq, kk), np.uint32), np.zeros(nq, np.uint64), np.zeros(nq, np.uint8)
        # a list of fetch_k entries is a truncated one -- unless fetch_k reaches the longest allowed set of the call: every list is whole
        max_m = len(self.base) if allows is None else max(int(allows[int(m)].sum()) for m in mask_of[:int(lims[-1])])
        trunc = None if fetch_k >= max_m else fetch_k
        for q in range(nq):
            w = None if weights is None else weights[int(lims[q]):int(lims[q + 1])]
            ids, sc, ex = R.fuse_groups(self.lists(kind, q, fetch_k, lims, allows, mask_of), self.group_of, k, mode, w, c, trunc_len=trunc)
            idx[q], bits[q], cnt[q] = fuse_ref.padded(ids + np.uint64(id_offset) if len(ids) else ids, sc, kk)
            exact[q] = ex
        return idx[:, :k], bits[:, :k], cnt, exact

    def direct(self, kind, q, lims, mode):
        """fused query q over the WHOLE table from the oracle's distance table, no lists: per group and sub-query the smallest distance
        (ties: the lower row); MIN -> the smallest over the sub-queries, SUM -> their f32 fold in sub-query order.  -> the groups'
        (score order key, representative row) pairs, ascending"""
        oi, od = self.full[kind]
        js = list(range(int(lims[q]), int(lims[q + 1])))
        best = {}  # group -> per sub-query (order key, row, distance)
        for s, j in enumerate(js):
            for row, d in zip(oi[j].tolist(), od[j]):  # (in the knn order: a group's first row is its nearest)
                best.setdefault(self.group_of(row), {}).setdefault(s, (R.order_key(d), row, d))
        out = []
        with np.errstate(all="ignore"):
            for g, per in best.items():
                rep = min((per[s][0], s, per[s][1]) for s in per)
                if mode == "min":
                    key = rep[0]
                else:
                    acc = np.float32(0.0)
                    for s in range(len(js)):
                        acc = np.float32(acc + per[s][2])
                    key = R.order_key(acc)
                out.append((key, rep[2]))
        return sorted(out)


@pytest.fixture(scope="module")
def sets():
    return {"random": Data(*_random_set()), "clustered": Data(*_clustered_set())}


def _same(got, exp, what=""):
    gi, gd, gc, ge = got
    ei, eb, ec, ee = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), (what, gi[:2], ei[:2])
    assert gd.dtype == np.float32 and np.array_equal(_canon(gd.view(np.uint32)), _canon(eb)), (what, gd[:2], eb.view(np.float32)[:2])
    assert np.array_equal(ge, ee), (what, ge, ee)


def _stats(ix, names=USTATS + FSTATS):
    return {s: ix.get_stat(s) for s in names}


def _delta(ix, s0):
    return {s: ix.get_stat(s) - v for s, v in s0.items()}


def _allow(n, ids):
    a = np.zeros(n, dtype=np.bool_)
    a[np.asarray(ids, dtype=np.int64)] = True
    return a


def _index(dist, D, n=None):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(D.base.shape[1], dist)
    ix.batch_add(D.base[:n])
    ix.set_labels(COL, D.labels[:n])
    return ix


def _device(ix, qs, lims, k, fetch_k, column=COL, **kw):
    import torch

    nq, kk = len(lims) - 1, max(k, 1)
    tq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    ti = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    td = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    tc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    te = torch.full((nq,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.flat_knn_fused_groups_device(tq.data_ptr(), lims, k, fetch_k, column, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), te.data_ptr(), **kw)
    finally:
        torch.cuda.synchronize()
        _device.last = (ti.cpu().numpy().view(np.uint64)[:, :k], td.cpu().numpy()[:, :k], tc.cpu().numpy().view(np.uint64), te.cpu().numpy())
    return _device.last


def test_the_group_answer_differs_from_the_row_level_answer_on_the_cpu(sets):
    """otherwise the comparisons below would show nothing: on the clustered set the nearest rows are several chunks of few documents"""
    D = sets["clustered"]
    differ = 0
    for q in range(len(SIZES)):
        lists = D.lists(0, q, 40, D.lims)
        rows, _ = fuse_ref.fuse(lists, 30, "rrf")
        reps, _, _ = R.fuse_groups(lists, D.group_of, 30, "rrf")
        docs = [D.group_of(r) for r in rows.tolist()]
        differ += len(set(docs)) < len(docs) and rows.tolist() != reps.tolist()
        assert len({D.group_of(r) for r in reps.tolist()}) == len(reps)
    assert differ == len(SIZES)  # every fused query: the row-level top 10 repeats a document, the group-level one cannot


@pytest.mark.parametrize("name", ("random", "clustered"))
@pytest.mark.parametrize("dist,kind", DISTS)
def test_cases_against_the_oracle(sets, name, dist, kind):
    D = sets[name]
    ix = _index(dist, D)
    try:
        w = np.random.default_rng(5).uniform(0.25, 4.0, size=len(D.qs)).astype(np.float32)
        for k, fetch_k in ((10, 10), (10, 40), (10, 65), (1, 1), (100, 300), (0, 5)):
            for mode, weights, c in (("rrf", None, 60.0), ("rrf", w, 0.0), ("min", None, 60.0), ("sum", None, 60.0)):
                got = ix.flat_knn_fused_groups(D.qs, D.lims, k, fetch_k, COL, mode, weights, c, return_exact=True)
                _same(got, D.expect(kind, k, fetch_k, mode, weights, c), f"{name} {dist} k={k} F={fetch_k} {mode}")
        got = ix.flat_knn_fused_groups(D.qs, D.lims, 10, 40, COL, "sum")  # the default return shape
        assert len(got) == 3 and np.array_equal(got[0], D.expect(kind, 10, 40, "sum")[0])
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_fetch_k_of_the_whole_table_is_the_true_answer(sets, dist, kind):
    D = sets["random"]
    ix = _index(dist, D)
    try:
        lims = _lims(SIZES_FULL)
        qs = D.qs[:int(lims[-1])]
        k = 700  # past the number of groups
        for mode in MODES:
            gi, gd, gc, ge = ix.flat_knn_fused_groups(qs, lims, k, N, COL, mode, return_exact=True)
            _same((gi, gd, gc, ge), D.expect(kind, k, N, mode, lims=lims), f"{dist} {mode} fetch_k = n")
            assert (ge == 1).all(), mode  # every list is the whole table
            assert not ix.flat_knn_fused_groups(qs, lims, k, N - 1, COL, mode, return_exact=True)[3].any(), mode  # ... one row short: cut
            if mode == "rrf":
                continue
            for q in range(len(SIZES_FULL)):
                exp = D.direct(kind, q, lims, mode)
                n = int(gc[q])
                assert n == len(exp) and gi[q, :n].tolist() == [r for _, r in exp], (dist, mode, q)
                assert [R.order_key(x) for x in gd[q, :n]] == [o for o, _ in exp], (dist, mode, q)
            assert np.isnan(gd[0, int(gc[0]) - 1])  # the unlabelled NaN row is a group of its own, last
    finally:
        ix.close()


@pytest.mark.parametrize("direct_max", (8192, 500))
def test_with_masks_on_both_routes(sets, direct_max):
    """masks up to flat_filtered_direct_max rows share the grouped launch, longer ones take the per-mask route"""
    D = sets["clustered"]
    ix = _index("l2sqr", D)
    try:
        ix.set_param("flat_filtered_direct_max", direct_max)
        nsub = len(D.qs)
        allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400)), _allow(N, [7, 27, 47, 1007, 2999]), _allow(N, []),
                  _allow(N, np.arange(N))]
        masks = [ix.make_mask(a) for a in allows]
        one = np.zeros(nsub, dtype=np.uint32)
        per = (np.arange(nsub) % 5).astype(np.uint32)   # some sub-queries see a short mask, some nothing at all
        none = np.full(nsub, 3, dtype=np.uint32)
        for mo, what in ((one, "one mask"), (per, "a mask per sub-query"), (none, "nothing allowed")):
            for k, fetch_k in ((10, 10), (10, 65), (5, 300)):
                for mode in MODES:
                    got = ix.flat_knn_fused_groups(D.qs, D.lims, k, fetch_k, COL, mode, masks=masks, mask_of=mo, return_exact=True)
                    _same(got, D.expect(0, k, fetch_k, mode, allows=allows, mask_of=mo), f"{what} k={k} F={fetch_k} {mode}")
        got = ix.flat_knn_fused_groups(D.qs, D.lims, 10, 64, COL, "sum", masks=masks[1], mask_of=None, return_exact=True)  # one RowMask for all
        _same(got, D.expect(0, 10, 64, "sum", allows=allows, mask_of=np.ones(nsub, dtype=np.uint32)), "single mask")
        gi, gd, gc, ge = ix.flat_knn_fused_groups(D.qs, D.lims, 10, 64, COL, "min", masks=masks, mask_of=none, return_exact=True)
        assert (gc == 0).all() and (ge == 1).all()  # nothing allowed: nothing cut
    finally:
        ix.close()


def test_counters_of_the_call_and_of_the_searches_under_it(sets):
    import torch

    D = sets["random"]
    nsub, nq = len(D.qs), len(SIZES)
    a, b = _index("l2sqr", D), _index("l2sqr", D)
    try:
        for fetch_k in (64, 65):
            tq = torch.from_numpy(D.qs).cuda()
            ti = torch.zeros((nsub, fetch_k), dtype=torch.int64, device="cuda")
            td = torch.zeros((nsub, fetch_k), dtype=torch.float32, device="cuda")
            tc = torch.zeros((nsub,), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            s0 = _stats(b)
            b.flat_knn_device(tq.data_ptr(), nsub, fetch_k, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
            under = _delta(b, s0)
            s0 = _stats(a)
            a.flat_knn_fused_groups(D.qs, D.lims, 10, fetch_k, COL, "sum")
            assert _delta(a, s0) == {**under, "flat_fused_groups_calls": 1, "flat_fused_groups_queries": nq, "flat_fused_groups_lists": nsub}, fetch_k
            allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400))]
            mo = (np.arange(nsub) % 2).astype(np.uint32)
            s0 = _stats(b)
            b.flat_knn_filtered_multi(D.qs, fetch_k, [b.make_mask(x) for x in allows], mo)
            under = _delta(b, s0)
            assert under["flat_filtered_multi_calls"] == 1
            s0 = _stats(a)
            a.flat_knn_fused_groups(D.qs, D.lims, 10, fetch_k, COL, "min", masks=[a.make_mask(x) for x in allows], mask_of=mo)
            assert _delta(a, s0) == {**under, "flat_fused_groups_calls": 1, "flat_fused_groups_queries": nq, "flat_fused_groups_lists": nsub}, fetch_k
        s0 = _stats(a)
        a.flat_knn_fused_groups(D.qs[:0], [0], 10, 40, COL)  # no fused query: a call all the same, nothing else
        gi, gd, gc, ge = a.flat_knn_fused_groups(D.qs, D.lims, 0, 40, COL, return_exact=True)  # k == 0: counted, no search under it
        assert (gc == 0).all() and (ge == 0).all()
        assert _delta(a, s0) == {**{s: 0 for s in FSTATS}, "flat_fused_groups_calls": 2, "flat_fused_groups_queries": nq, "flat_fused_groups_lists": nsub}
        a.prof_enable(True)
        a.prof_reset()
        a.flat_knn_fused_groups(D.qs, D.lims, 10, 40, COL)
        p = a.prof_get("fuse_groups")
        assert p["launches"] == 1 and p["ms"] > 0, p
        assert a.prof_get("fuse_lists")["launches"] == 0
    finally:
        a.close()
        b.close()


def test_device_form_id_offset_and_a_never_written_column(sets):
    D = sets["clustered"]
    ix = _index("cosine", D)
    try:
        w = np.linspace(0.5, 2.0, len(D.qs)).astype(np.float32)
        allows = [_allow(N, np.arange(0, N, 2)), _allow(N, np.arange(0, 400))]
        masks = [ix.make_mask(x) for x in allows]
        mo = (np.arange(len(D.qs)) % 2).astype(np.uint32)
        for off in (0, (1 << 33) + 3):
            ix.set_id_offset(off)
            _same(_device(ix, D.qs, D.lims, 10, 40, mode="rrf", weights=w, rrf_c=1.0), D.expect(1, 10, 40, "rrf", w, 1.0, id_offset=off), "device rrf")
            _same(_device(ix, D.qs, D.lims, 80, 80, mode="sum"), D.expect(1, 80, 80, "sum", id_offset=off), "device sum")
            _same(_device(ix, D.qs, D.lims, 10, 65, mode="min", masks=masks, mask_of=mo),
                  D.expect(1, 10, 65, "min", allows=allows, mask_of=mo, id_offset=off), "device masks")
        ix.set_id_offset(0)
        gi, gd, gc, ge = _device(ix, D.qs, D.lims, 0, 0)  # k == 0: counts only, no slot touched
        assert (gc == 0).all() and (ge == 0).all()
        # a column never written: every row a group of its own -- the row-level fused search, bit for bit
        for mode in ("rrf", "min"):
            a = ix.flat_knn_fused_groups(D.qs, D.lims, 10, 40, 9, mode)
            b = ix.flat_knn_fused(D.qs, D.lims, 10, 40, mode)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    finally:
        ix.close()


def test_refused_calls_leave_outputs_and_every_counter(sets):
    import lab_1806_vec_db_amd as vdb

    D = sets["random"]
    ix = _index("l2sqr", D)
    other = _index("l2sqr", D, 100)
    try:
        mk, foreign = ix.make_mask(np.arange(50)), other.make_mask(np.arange(50))
        nsub = len(D.qs)
        s0 = _stats(ix)

        def refused(match, *a, exc=vdb.VdbError, lims=D.lims, qs=D.qs, column=COL, **kw):
            with pytest.raises(exc, match=match):
                _device(ix, qs, lims, *a, column=column, **kw)
            gi, gd, gc, ge = _device.last
            assert (gi == SENT).all() and (gd == -7.0).all() and (gc == SENT).all() and (ge == 77).all(), match
            with pytest.raises(exc, match=match):
                ix.flat_knn_fused_groups(qs, lims, *a, column, **kw)

        refused("mode", 10, 40, mode=3)
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
        refused("VDB_FUSE_RRF only", 10, 40, mode="min", weights=np.ones(nsub))
        refused("no weighted VDB_FUSE_SUM", 10, 40, mode="sum", weights=np.ones(nsub))
        for c in (-1.0, float("nan"), float("inf")):
            refused("rrf_c", 10, 40, rrf_c=c)
        refused("VDB_LABEL_COLUMNS", 10, 40, column=16)
        refused("mask_of", 10, 40, masks=[mk], mask_of=np.full(nsub, 1, dtype=np.uint32))
        refused("mask", 10, 40, masks=[foreign], mask_of=np.zeros(nsub, dtype=np.uint32))
        assert _delta(ix, s0) == {s: 0 for s in s0}
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.flat_knn_fused_groups(np.zeros((nsub, DIM + 1), np.float32), D.lims, 10, 40, COL)
        with pytest.raises(ValueError, match="fusion mode"):
            ix.flat_knn_fused_groups(D.qs, D.lims, 10, 40, COL, "max")
        with pytest.raises(ValueError, match="fusion mode"):
            ix.flat_knn_fused(D.qs, D.lims, 10, 40, "sum")  # the row-level search has no sum
        ix.batch_add(D.base[:1])  # the mask is stale now
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.flat_knn_fused_groups(D.qs, D.lims, 10, 40, COL, masks=[mk], mask_of=np.zeros(nsub, dtype=np.uint32))
        assert _delta(ix, s0) == {s: 0 for s in s0}
        u8 = vdb.GpuIndex(DIM, "l2sqr", scalar="u8")
        try:
            u8.batch_add_u8(np.zeros((8, DIM), dtype=np.uint8))
            with pytest.raises(vdb.VdbError, match="f32 rows"):
                u8.flat_knn_fused_groups(np.zeros((2, DIM), np.float32), [0, 2], 1, 4, COL)
        finally:
            u8.close()
    finally:
        ix.close()
        other.close()
