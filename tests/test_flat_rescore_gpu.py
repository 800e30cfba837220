"""GPU: the exact late-interaction rescoring of candidate documents (GpuIndex.rescore_groups / rescore_groups_device,
vdb_flat_rescore_groups*) on 575 rows whose label groups hold 1, 63, 64, 65 and 150 rows (a group ends at, starts at and spans a tile of 64
entries), interleaved over the table, with unlabelled rows, identical rows, a NaN row inside a group and a group of NaN rows only.  The
pair distances are the CPU oracle's (oracle.flat_knn_batch at k = n); the reference (tests/rescore_ref.py) takes per group and sub-query
the smallest under (distance, row) with NaN last, folds a strict np.float32 sum over the sub-queries and sorts by (score, representative).
The criterion is equality of bits (NaN scores compare as NaN).  One shape only: tests/test_flat_rescore_shapes_gpu.py goes past it."""
import numpy as np
import pytest

import rescore_ref

pytestmark = pytest.mark.gpu

NONE, COL, LD = 0xFFFFFFFF, 3, 16
SIZES = (1, 4, 5, 32)      # sub-queries per question: 5 gives wave 0 a second one, 32 fills the accumulators
COUNTS = (6, 9, 14, 16)    # candidates per question, of the one list CANDS below
STATS = ("flat_rescore_calls", "flat_rescore_questions", "flat_rescore_rows")
SENT = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)
LIMS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)


def _labels():
    lab = np.concatenate([np.full(c, v) for v, c in ((10, 1), (11, 63), (12, 64), (13, 65), (14, 150), (15, 3), (16, 8), (NONE, 21))]
                         + [100 + np.arange(200) // 6]).astype(np.uint32)
    return lab[np.random.default_rng(91).permutation(len(lab))]


LAB = _labels()
N = len(LAB)
ROWS_OF = {int(v): np.flatnonzero(LAB == v) for v in np.unique(LAB)}
# the first of 11, of 12, ANOTHER of 11 (one group: counts once), an unlabelled row, the NaN-only group, 13 | 14, 16, 10 | ...
CANDS = np.array([ROWS_OF[11][0], ROWS_OF[12][5], ROWS_OF[11][40], ROWS_OF[NONE][0], ROWS_OF[15][1], ROWS_OF[13][64], ROWS_OF[14][149],
                  ROWS_OF[16][7], ROWS_OF[10][0], ROWS_OF[NONE][20], ROWS_OF[100][3], ROWS_OF[14][0], ROWS_OF[101][0], ROWS_OF[NONE][7],
                  ROWS_OF[120][2], ROWS_OF[133][1]], dtype=np.uint64)


class Data:
    def __init__(self, dim):
        from oracle import oracle as O

        rng = np.random.default_rng(9000 + dim)
        self.base = rng.random((N, dim)).astype(np.float32)
        self.base[ROWS_OF[16][:5]] = self.base[ROWS_OF[16][0]]  # identical rows in one group: the lower row represents it
        self.base[ROWS_OF[15], 0] = np.nan                      # a group of NaN rows only
        self.base[ROWS_OF[14][3], dim - 1] = np.nan             # a NaN row inside a group
        self.qs = rng.random((int(LIMS[-1]), dim)).astype(np.float32)
        self.qs[1] = self.base[ROWS_OF[13][2]]                  # a sub-query equal to a stored row
        self.dm = {}
        for kind in (0, 1):  # the dense distance table, computed once, shared, never changed
            oi, od, oc = O.flat_knn_batch(self.base, self.qs, N, kind, nthreads=16)
            assert (oc == N).all()
            self.dm[kind] = np.zeros((len(self.qs), N), np.float32)
            np.put_along_axis(self.dm[kind], oi.astype(np.int64), od, axis=1)

    def expect(self, kind, k, mode, labels=LAB, allows=None, mask_of=None, off=0, counts=COUNTS):
        """-> (idx, score bits, count, candidate rows evaluated) of tests/rescore_ref.py"""
        cand, cnt = _cands(off, counts)
        return rescore_ref.expect(self.dm[kind], labels, LIMS, cand, cnt, k, mode, allows=allows, mask_of=mask_of, id_offset=off)


@pytest.fixture(scope="module", params=(1, 3, 4, 33, 130))  # the element-wise tail, a 32-slice boundary, several slices with a tail
def data(request):
    return Data(request.param)


def _same(got, exp, what):
    _canon = lambda b: np.where((b & 0x7FFFFFFF) > 0x7F800000, np.uint32(0x7FC00000), b)  # noqa: E731  (NaN scores compare as NaN)
    assert np.array_equal(got[2], exp[2]), (what, got[2], exp[2])
    assert np.array_equal(got[0], exp[0]), (what, got[0], exp[0])
    assert got[1].dtype == np.float32 and np.array_equal(_canon(got[1].view(np.uint32)), _canon(exp[1])), (what, got[1], exp[1].view(np.float32))


def _index(dist, D):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(D.base.shape[1], dist)
    ix.batch_add(D.base)
    ix.set_labels(COL, LAB)
    return ix


def _cands(off=0, counts=COUNTS):
    return np.tile(CANDS + np.uint64(off), (len(SIZES), 1)), np.array(counts, dtype=np.uint64)


def _device(ix, qs, lims, cand, cnt, k, column=COL, ld=LD, **kw):
    import torch

    nq, kk, tq = len(lims) - 1, max(k, 1), torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    tci, tcc = torch.from_numpy(cand.view(np.int64)).cuda(), torch.from_numpy(cnt.view(np.int64)).cuda()
    ti = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    td = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    tc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.rescore_groups_device(tq.data_ptr(), lims, tci.data_ptr(), tcc.data_ptr(), ld, k, column, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), **kw)
    finally:
        torch.cuda.synchronize()
        _device.last = (ti.cpu().numpy().view(np.uint64)[:, :k], td.cpu().numpy()[:, :k], tc.cpu().numpy().view(np.uint64))
    return _device.last


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_both_forms_against_the_reference(data, dist, kind):
    D = data
    ix = _index(dist, D)
    try:
        nsub = len(D.qs)
        hide = np.ones(N, dtype=np.bool_)
        hide[ROWS_OF[12]] = False  # a sub-query under this mask allows no row of group 12: +inf under SUM, ignored under MIN
        allows = [hide, np.ones(N, dtype=np.bool_), np.arange(N) % 3 != 0]
        masks = [ix.make_mask(a) for a in allows]
        mo = (np.arange(nsub) % 3).astype(np.uint32)
        mo[0] = 0  # question 0 has ONE sub-query: group 12 has no allowed row at all, its candidate represents it
        for mode in ("sum", "min"):
            for off in (0, (1 << 33) + 3):
                ix.set_id_offset(off)
                cand, cnt = _cands(off)
                for k in (16, 3):  # 16: above the number of distinct groups of every question
                    s0 = {s: ix.get_stat(s) for s in STATS}
                    exp = D.expect(kind, k, mode, off=off)
                    host = ix.rescore_groups(D.qs, LIMS, cand, cnt, k, COL, mode)
                    _same(host, exp, f"{dist} {mode} k={k} off={off}")
                    assert {s: ix.get_stat(s) - v for s, v in s0.items()} == dict(zip(STATS, (1, len(SIZES), exp[3])))
                    dev = _device(ix, D.qs, LIMS, cand, cnt, k, mode=mode)
                    again = _device(ix, D.qs, LIMS, cand, cnt, k, mode=mode)
                    for a, b, c in zip(host, dev, again):  # the device form matches the host form; two calls return the same bits
                        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(b.view(np.uint32), c.view(np.uint32))
                exp = D.expect(kind, 16, mode, allows=allows, mask_of=mo, off=off)
                _same(ix.rescore_groups(D.qs, LIMS, cand, cnt, 16, COL, mode, masks=masks, mask_of=mo), exp, f"{dist} {mode} masks")
                _same(_device(ix, D.qs, LIMS, cand, cnt, 16, mode=mode, masks=masks, mask_of=mo), exp, f"{dist} {mode} masks, device")
                assert np.isinf(exp[1].view(np.float32)).any()
            ix.set_id_offset(0)
            cand, cnt = _cands()
            # a column never written: every candidate row is a group of its own
            _same(ix.rescore_groups(D.qs, LIMS, cand, cnt, 16, 9, mode), D.expect(kind, 16, mode, labels=np.full(N, NONE, np.uint32)), "no column")
            s0 = ix.get_stat("flat_rescore_rows")
            gi, gd, gc = _device(ix, D.qs, LIMS, cand, cnt, 0, mode=mode)  # k == 0: counts only, no pair evaluated
            assert (gc == 0).all() and ix.get_stat("flat_rescore_rows") == s0
            gi, gd, gc = ix.rescore_groups(D.qs, LIMS, cand, np.zeros(len(SIZES), np.uint64), 4, COL, mode)  # no candidates
            assert (gc == 0).all() and (gi == 0).all() and (gd == 0).all() and ix.get_stat("flat_rescore_rows") == s0
    finally:
        ix.close()


def test_refused_calls_leave_outputs_and_counters(data):
    import lab_1806_vec_db_amd as vdb

    D = data
    dim = D.base.shape[1]
    ix = _index("l2sqr", D)
    other, u8 = vdb.GpuIndex(dim, "l2sqr"), vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    other.batch_add(D.base[:100])
    try:
        mk, foreign = ix.make_mask(np.arange(50)), other.make_mask(np.arange(50))
        nsub = len(D.qs)
        cand, cnt = _cands()
        s0 = {s: ix.get_stat(s) for s in STATS}

        def refused(match, k=4, lims=LIMS, qs=D.qs, cand=cand, cnt=cnt, column=COL, ld=LD, host=True, **kw):
            with pytest.raises(vdb.VdbError, match=match):
                _device(ix, qs, lims, cand, cnt, k, column=column, ld=ld, **kw)
            gi, gd, gc = _device.last
            assert (gi == SENT).all() and (gd == -7.0).all() and (gc == SENT).all(), match
            if host:
                with pytest.raises(vdb.VdbError, match=match):
                    ix.rescore_groups(qs, lims, cand, cnt, k, column, **kw)

        refused("mode", mode="rrf")
        refused("VDB_LABEL_COLUMNS", column=16)
        refused("at least one sub-query", lims=np.concatenate([LIMS[:3], LIMS[2:]]), cand=np.tile(CANDS, (5, 1)), cnt=np.zeros(5, np.uint64))
        refused("at most 32", lims=np.array([0, 33], dtype=np.uint64), qs=np.zeros((33, dim), np.float32), cand=cand[:1], cnt=cnt[:1])
        refused("at most 4096", ld=4097, host=False)
        refused("k must be at most ld", k=17)
        refused("above ld", cnt=np.array([6, 17, 1, 1], dtype=np.uint64))
        bad = cand.copy()
        bad[2, 5] = N  # a counted id that is no row, found on the device
        refused("no row of this index", cand=bad)
        refused("mask_of", masks=[mk], mask_of=np.full(nsub, 1, dtype=np.uint32))
        refused("mask", masks=[foreign], mask_of=np.zeros(nsub, dtype=np.uint32))
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.rescore_groups(np.zeros((nsub, dim + 1), np.float32), LIMS, cand, cnt, 4, COL)
        ix.batch_add(D.base[:1])  # the mask is stale now
        with pytest.raises(vdb.VdbError, match="error 3.*stale"):
            ix.rescore_groups(D.qs, LIMS, cand, cnt, 4, COL, masks=[mk], mask_of=np.zeros(nsub, dtype=np.uint32))
        u8.batch_add_u8(np.zeros((8, dim), dtype=np.uint8))
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            u8.rescore_groups(np.zeros((2, dim), np.float32), [0, 2], [[0, 1]], [2], 1, COL)
        assert {s: ix.get_stat(s) - v for s, v in s0.items()} == {s: 0 for s in STATS}
    finally:
        ix.close()
        other.close()
        u8.close()
