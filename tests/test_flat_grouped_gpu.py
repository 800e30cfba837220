"""GPU: grouped Flat k-NN (GpuIndex.flat_knn_grouped, vdb_flat_knn_grouped: at most g hits per value of one label column) end to end
against the CPU oracle.

The expected answer of a query is the oracle's full order -- oracle.flat_knn_batch(base, qs, len(base), kind): every row in the
reference's (distance, index) order, NaN distances last -- restricted to the rows the query's mask allows and walked by _walk below:
an unlabelled row is kept, a row with label v iff fewer than g earlier rows of that order carry v; the first k kept.  Every case is
bit-exact: ids equal, distances equal as f32 bit patterns, counts equal, slots past the count zero."""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
NONE = 0xFFFFFFFF
GSTATS = ("flat_grouped_calls", "flat_grouped_queries", "flat_grouped_rounds", "flat_grouped_exhausted_queries")
FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries",
          "flat_filtered_multi_calls", "flat_filtered_grouped_queries", "flat_fallback", "flat_i8_queries", "flat_half_queries")
N = 3000
COL_DOC, COL_SKEW, COL_NEVER = 0, 1, 7


# (a copy of the helper of tests/test_flat_filtered_gpu.py)
def _full_order(base, qs, kind):
    """(ids, distances) of every row per query in the reference's order (NaN distances last)"""
    from oracle import oracle as O

    oi, od, oc = O.flat_knn_batch(base, qs, len(base), kind, nthreads=16)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _walk(codes, g, k):
    """positions kept from the codes of a query's order"""
    kept, seen = [], {}
    for p, c in enumerate(codes.tolist()):
        if len(kept) == k:
            break
        if c != NONE:
            if seen.get(c, 0) >= g:
                continue
            seen[c] = seen.get(c, 0) + 1
        kept.append(p)
    return kept


def _expect(full, labels, k, g, allows=None, mask_of=None, id_offset=0):
    oi, od = full
    nq, kk = len(oi), max(k, 1)
    idx = np.zeros((nq, kk), dtype=np.uint64)
    dist = np.zeros((nq, kk), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        rows, d = oi[q].astype(np.int64), od[q]
        if allows is not None:
            keep = allows[int(mask_of[q])][rows]
            rows, d = rows[keep], d[keep]
        kept = _walk(labels[rows], g, k)
        cnt[q] = len(kept)
        idx[q, :len(kept)] = rows[kept].astype(np.uint64) + np.uint64(id_offset)
        dist[q, :len(kept)] = d[kept]
    return idx[:, :k], dist[:, :k], cnt


def _same(got, exp, what=""):
    gi, gd, gc = got
    ei, ed, ec = exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), what
    assert gd.dtype == np.float32 and np.array_equal(np.isnan(gd), np.isnan(ed)), what  # (a NaN's payload is not part of the contract)
    ok = ~np.isnan(ed)
    assert np.array_equal(gd[ok].view(np.uint32), ed[ok].view(np.uint32)), what


def _stats(ix, names=GSTATS + FSTATS):
    return {s: ix.get_stat(s) for s in names}


def _delta(ix, s0):
    return {s: ix.get_stat(s) - v for s, v in s0.items()}


def _allow(n, ids):
    a = np.zeros(n, dtype=np.bool_)
    a[np.asarray(ids, dtype=np.int64)] = True
    return a


def _labels():
    rng = np.random.default_rng(2301)
    doc = (rng.permutation(N) % 300).astype(np.uint32)  # 300 values x 10 rows
    skew = np.full(N, 5, dtype=np.uint32)               # 2700 rows under one value, 300 under values of their own
    lone = rng.choice(N, 300, replace=False)
    skew[lone] = 1000 + np.arange(300, dtype=np.uint32)
    return {COL_DOC: doc, COL_SKEW: skew, COL_NEVER: np.full(N, NONE, dtype=np.uint32)}


@pytest.fixture(scope="module")
def small():
    """3000 x 960 gist-like rows, 9 queries, both metrics' full orders (computed once, never changed)"""
    base = gist_like(N, seed=2301)
    qs = gist_like(9, seed=2302)
    return base, qs, {kind: _full_order(base, qs, kind) for _, kind in DISTS}, _labels()


def _index(dist, base, labels, mode=None):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist)
    ix.batch_add(base)
    for c in (COL_DOC, COL_SKEW):
        ix.set_labels(c, labels[c])
    if mode is not None:
        ix.set_flat_mode(mode)
    return ix


@pytest.mark.parametrize("dist,kind", DISTS)
def test_columns_group_sizes_and_k(small, dist, kind):
    base, qs, fulls, labels = small
    full = fulls[kind]
    ix = _index(dist, base, labels)
    try:
        for col in (COL_DOC, COL_SKEW):
            for g in (1, 2, 10):
                for k in (1, 10, 100):
                    s0 = _stats(ix, GSTATS)
                    got = ix.flat_knn_grouped(qs, k, col, g)
                    d = _delta(ix, s0)
                    _same(got, _expect(full, labels[col], k, g), (dist, col, g, k))
                    assert d["flat_grouped_calls"] == 1 and d["flat_grouped_queries"] == len(qs) and d["flat_grouped_rounds"] >= 1, d
                    if col == COL_SKEW and k >= 10 and g <= 2:  # 9 of 10 candidates carry one value: the first list keeps too few, the call goes round again
                        assert d["flat_grouped_rounds"] > 1, d
        # only 301 rows can ever be kept with g = 1: every query walks its whole table and the answer is short
        s0 = _stats(ix, GSTATS)
        got = ix.flat_knn_grouped(qs, 400, COL_SKEW, 1)
        d = _delta(ix, s0)
        _same(got, _expect(full, labels[COL_SKEW], 400, 1), (dist, "exhausted"))
        assert (got[2] == 301).all() and d["flat_grouped_exhausted_queries"] == len(qs) and d["flat_grouped_rounds"] > 1, d
        # one query, as flat_knn returns one
        gi, gd = ix.flat_knn_grouped(qs[3], 10, COL_DOC, 1)
        ei, ed, ec = _expect((full[0][3:4], full[1][3:4]), labels[COL_DOC], 10, 1)
        assert np.array_equal(gi, ei[0]) and np.array_equal(gd.view(np.uint32), ed[0].view(np.uint32))
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_unlimited_group_and_never_written_column(small, dist, kind):
    """a cap no group reaches, and a column never written: flat_knn's answer at the same k, bit for bit"""
    base, qs, fulls, labels = small
    ix = _index(dist, base, labels)
    try:
        for k in (1, 10, 100, 1500):
            plain = ix.flat_knn(qs, k)
            _same(plain, _expect(fulls[kind], labels[COL_NEVER], k, 1), (dist, k, "oracle"))
            for col, g in ((COL_DOC, 10), (COL_DOC, 1 << 40), (COL_SKEW, 2700), (COL_NEVER, 1)):
                _same(ix.flat_knn_grouped(qs, k, col, g), plain, (dist, k, col, g))
        assert ix.get_stat("label_columns") == 2
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_duplicate_rows_and_nan_rows(dist, kind):
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(41)
    base = rng.random((300, 64)).astype(np.float32)
    base[5, 17] = np.nan       # NaN distance to every query: sorts last
    base[77, 3] = np.nan
    base[20:30] = base[3]      # ties, decided by id
    qs = np.concatenate([rng.random((5, 64)).astype(np.float32), base[3:4]])
    full = _full_order(base, qs, kind)
    labels = (np.arange(300) % 7).astype(np.uint32)
    labels[20:30] = [1, 1, 2, 2, 2, 3, NONE, 1, 2, 3]  # equal rows under different labels
    labels[3] = 2
    labels[5], labels[77] = 4, 4                          # the NaN rows share a label
    ix = vdb.GpuIndex(64, dist)
    try:
        ix.batch_add(base)
        ix.set_labels(2, labels)
        for g in (1, 2, 50):
            for k in (1, 5, 11, 300):
                _same(ix.flat_knn_grouped(qs, k, 2, g), _expect(full, labels, k, g), (dist, g, k))
        gi, gd, gc = ix.flat_knn_grouped(qs[5:6], 6, 2, 1)  # the query IS row 3: labels 2 (row 3), 1 (20), - (22..24: 2), 3 (25), NONE (26)
        assert gi[0, :4].tolist() == [3, 20, 25, 26]
        gi, gd, gc = ix.flat_knn_grouped(qs, 300, 2, 50)   # no group reaches 50 rows: every row, both NaN rows last
        assert (gc == 300).all() and (np.sort(gi[:, -2:], axis=1) == [5, 77]).all() and np.isnan(gd[:, -2:]).all()
    finally:
        ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_with_masks(small, dist, kind):
    """one mask for every query, and a mask per query -- an empty one and one shorter than k among them"""
    base, qs, fulls, labels = small
    full = fulls[kind]
    rng = np.random.default_rng(8)
    allows = [_allow(N, rng.choice(N, 1200, replace=False)), _allow(N, []), _allow(N, rng.choice(N, 5, replace=False)),
              _allow(N, np.flatnonzero(labels[COL_SKEW] == 5)[:700]), np.ones(N, dtype=np.bool_)]
    ix = _index(dist, base, labels)
    try:
        masks = [ix.make_mask(a) for a in allows]
        zero = np.zeros(len(qs), dtype=np.uint32)
        for col in (COL_DOC, COL_SKEW):
            for g, k in ((1, 10), (2, 10), (1, 100)):
                s0 = _stats(ix, GSTATS + ("flat_filtered_multi_calls",))
                got = ix.flat_knn_grouped(qs, k, col, g, masks[0])
                d = _delta(ix, s0)
                _same(got, _expect(full, labels[col], k, g, allows[:1], zero), (dist, col, g, k, "one mask"))
                assert d["flat_filtered_multi_calls"] == d["flat_grouped_rounds"] >= 1, d
                mask_of = (np.arange(len(qs)) * 3 % len(masks)).astype(np.uint32)
                got = ix.flat_knn_grouped(qs, k, col, g, masks, mask_of)
                exp = _expect(full, labels[col], k, g, allows, mask_of)
                _same(got, exp, (dist, col, g, k, "mask per query"))
                assert (got[2][mask_of == 1] == 0).all() and (got[2][mask_of == 2] <= 5).all()
        # a mask whose every row carries one value, g = 1: one hit, after the whole mask was walked
        s0 = _stats(ix, GSTATS)
        got = ix.flat_knn_grouped(qs, 10, COL_SKEW, 1, masks[3])
        d = _delta(ix, s0)
        _same(got, _expect(full, labels[COL_SKEW], 10, 1, allows[3:4], zero), "one value")
        assert (got[2] == 1).all() and d["flat_grouped_exhausted_queries"] == len(qs), d
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_mode_2_under_a_long_mask_agrees_with_mode_1():
    """30 000 rows, a mask of 20 000: round 0 (K' <= 64) takes the filtered call's 8-bit tier in mode 2, later rounds (K' > 64) its direct
    path; the answers are those of mode 1, where everything is the direct path"""
    import lab_1806_vec_db_amd as vdb

    nb = 30000
    base = gist_like(nb, seed=2311)
    qs = gist_like(20, seed=2312)
    rng = np.random.default_rng(12)
    allow = _allow(nb, rng.choice(nb, 20000, replace=False))
    labels = np.where(rng.random(nb) < 0.8, 9, rng.integers(100, 4000, nb)).astype(np.uint32)
    ix = vdb.GpuIndex(960, "l2sqr")
    try:
        ix.batch_add(base)
        ix.set_labels(0, labels)
        mk = ix.make_mask(allow)
        out = {}
        for mode in (2, 1):
            ix.set_flat_mode(mode)
            s0 = _stats(ix)
            out[mode] = [ix.flat_knn_grouped(qs, 10, 0, g, mk) for g in (1, 3)] + [ix.flat_knn_grouped(qs, 10, 0, 1)]
            d = _delta(ix, s0)
            print(mode, d)
            assert (d["flat_filtered_i8_queries"] > 0) == (mode == 2), d
            assert d["flat_grouped_rounds"] > 3, d  # (8 of 10 candidates under one value: the first list does not hold 10 groups)
        for a, b in zip(out[2], out[1]):
            _same(a, b, "mode 2 vs mode 1")
        # ... and mode 1's answer is the walk of the filtered search's own long list
        li, ld, lc = ix.flat_knn_filtered(qs, 2000, mk)
        for q in range(len(qs)):
            kept = _walk(labels[li[q].astype(np.int64)], 1, 10)
            assert len(kept) == 10 and out[1][0][0][q].tolist() == li[q][kept].tolist()
            assert np.array_equal(out[1][0][1][q].view(np.uint32), ld[q][kept].view(np.uint32))
        mk.close()
    finally:
        ix.close()


def test_oversample_changes_rounds_not_answers(small):
    base, qs, fulls, labels = small
    ix = _index("l2sqr", base, labels)
    try:
        got, rounds = {}, {}
        for ov in (1, 4, 16):
            ix.set_param("flat_grouped_oversample", ov)
            s0 = _stats(ix, GSTATS)
            got[ov] = [ix.flat_knn_grouped(qs, 10, col, g) for col in (COL_DOC, COL_SKEW) for g in (1, 2)]
            rounds[ov] = _delta(ix, s0)["flat_grouped_rounds"]
        for a, b, c in zip(got[1], got[4], got[16]):
            _same(a, b, "oversample 1 vs 4")
            _same(a, c, "oversample 1 vs 16")
        _same(got[1][2], _expect(fulls[0], labels[COL_SKEW], 10, 1), "oracle")
        assert rounds[1] > rounds[16] >= 4 and rounds[1] >= rounds[4] >= rounds[16], rounds  # (four calls, at least a round each)
        import lab_1806_vec_db_amd as vdb

        with pytest.raises(vdb.VdbError):
            ix.set_param("flat_grouped_oversample", 0)
    finally:
        ix.close()


def test_refused_calls_leave_every_counter(small):
    import lab_1806_vec_db_amd as vdb

    base, qs, fulls, labels = small
    ix = _index("l2sqr", base, labels)
    other = _index("l2sqr", base[:100], {c: v[:100] for c, v in labels.items()})
    u8 = vdb.GpuIndex(960, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8((base[:50] * 255).astype(np.uint8))
        mk = ix.make_mask(_allow(N, range(100)))
        foreign = other.make_mask(_allow(100, range(10)))
        stale_ix = _index("l2sqr", base[:200], {c: v[:200] for c, v in labels.items()})
        stale = stale_ix.make_mask(_allow(200, range(50)))
        stale_ix.batch_add(base[200:210])
        s0, s0_stale, s0_u8 = _stats(ix), _stats(stale_ix), _stats(u8)
        zero = np.zeros(len(qs), dtype=np.uint32)
        bad = [
            (ix, dict(k=10, column=COL_DOC, group_size=0), "group_size"),
            (ix, dict(k=10, column=16, group_size=1), "column"),
            (u8, dict(k=10, column=0, group_size=1), "f32 rows"),
            (ix, dict(k=10, column=COL_DOC, group_size=1, masks=[mk, foreign], mask_of=zero), None),
            (stale_ix, dict(k=10, column=COL_DOC, group_size=1, masks=[stale], mask_of=zero), "error 3.*stale"),
            (ix, dict(k=10, column=COL_DOC, group_size=1, masks=[mk], mask_of=zero + 1), "mask_of"),
        ]
        for index, kw, match in bad:
            with pytest.raises(vdb.VdbError, match=match):
                index.flat_knn_grouped(qs, **kw)
        with pytest.raises(vdb.VdbError, match="dimension"):
            ix.flat_knn_grouped(qs[:, :100], 10, COL_DOC, 1)
        assert _stats(ix) == s0 and _stats(stale_ix) == s0_stale and _stats(u8) == s0_u8
        # empty results: no queries, k = 0, nothing allowed
        gi, gd, gc = ix.flat_knn_grouped(qs[:0], 10, COL_DOC, 1)
        assert gi.shape[0] == 0 and gc.shape == (0,)
        gi, gd, gc = ix.flat_knn_grouped(qs, 0, COL_DOC, 1)
        assert (gc == 0).all()
        empty = ix.make_mask(_allow(N, []))
        gi, gd, gc = ix.flat_knn_grouped(qs, 10, COL_DOC, 1, empty)
        assert (gc == 0).all() and (gi == 0).all() and (gd == 0).all()
        for m in (mk, foreign, stale, empty):
            m.close()
        stale_ix.close()
    finally:
        u8.close()
        other.close()
        ix.close()


def test_device_form(small):
    import torch

    base, qs, fulls, labels = small
    ix = _index("cosine", base, labels)
    try:
        ix.set_id_offset(50000)
        nq, k = len(qs), 10
        allows = [_allow(N, range(0, N, 2)), _allow(N, range(1, N, 2))]
        masks = [ix.make_mask(a) for a in allows]
        mask_of = (np.arange(nq) % 2).astype(np.uint32)
        tq = torch.from_numpy(qs).cuda()
        for use_masks in (False, True):
            ti = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
            td = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
            tc = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if use_masks:
                ix.flat_knn_grouped_device(tq.data_ptr(), nq, k, COL_SKEW, 2, ti.data_ptr(), td.data_ptr(), tc.data_ptr(), masks, mask_of)
                exp = _expect(fulls[1], labels[COL_SKEW], k, 2, allows, mask_of, id_offset=50000)
            else:
                ix.flat_knn_grouped_device(tq.data_ptr(), nq, k, COL_SKEW, 2, ti.data_ptr(), td.data_ptr(), tc.data_ptr())
                exp = _expect(fulls[1], labels[COL_SKEW], k, 2, id_offset=50000)
            torch.cuda.synchronize()
            _same((ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().view(np.uint64)), exp, ("device", use_masks))
        for m in masks:
            m.close()
    finally:
        ix.close()


def test_two_threads(small):
    base, qs, fulls, labels = small
    ix = _index("l2sqr", base, labels)
    try:
        exp = {t: _expect(fulls[0], labels[(COL_DOC, COL_SKEW)[t]], 10, 1 + t) for t in range(2)}
        errs = []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(4):
                    _same(ix.flat_knn_grouped(qs, 10, (COL_DOC, COL_SKEW)[t], 1 + t), exp[t], ("thread", t))
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        assert ix.get_stat("flat_grouped_calls") == 8
    finally:
        ix.close()
