"""GPU: k_like_drop alone (GpuIndex.drop_listed_device, vdb_drop_listed_device) over hand-made lists against like_ref.drop_listed (verified
on the CPU by tests/test_like_ref_cpu.py).  The lists are walked as given -- any order of ids, any distances -- and every comparison is
exact: ids, order, distances as f32 bit patterns (the kernel only moves them), counts, zeros behind the count."""
import numpy as np
import pytest

import like_ref as R

pytestmark = pytest.mark.gpu

N = 1500
LDS = (1, 63, 64, 65, 128, 200)


@pytest.fixture(scope="module")
def ix():
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(4, "l2sqr", device=0)
    ix.batch_add(np.random.default_rng(1).standard_normal((N, 4)).astype(np.float32))
    yield ix
    ix.close()


def _run(ix, lists, ld, k, drops, id_offset=0, counts=None, dists=None):
    """lists / drops: per query LOCAL rows -> (idx, dist, cnt) from the device, outputs pre-filled with a sentinel"""
    import torch

    nq = len(lists)
    ids = np.full((nq, max(ld, 1)), 0xDEAD00, dtype=np.uint64)  # (beyond a count: never read -- no row at all)
    dd = np.full((nq, max(ld, 1)), -3.0, dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q, rows in enumerate(lists):
        ids[q, :len(rows)] = np.asarray(rows, dtype=np.uint64) + np.uint64(id_offset)
        dd[q, :len(rows)] = dists[q] if dists is not None else np.arange(len(rows), dtype=np.float32) * np.float32(0.37) + np.float32(q)
        cnt[q] = len(rows)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.uint64)
    lims = np.concatenate([[0], np.cumsum([len(x) for x in drops])]).astype(np.uint64)
    flat = np.asarray([r for x in drops for r in x], dtype=np.uint64) + np.uint64(id_offset)
    kk = max(k, 1)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(dd).cuda()
    t_c = torch.from_numpy(cnt.view(np.int64)).cuda()
    t_x = torch.from_numpy(flat.view(np.int64)).cuda()
    o_i = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.drop_listed_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), nq, ld, k, lims, t_x.data_ptr() if len(flat) else 0, o_i.data_ptr(),
                              o_d.data_ptr(), o_c.data_ptr())
    finally:
        torch.cuda.synchronize()
        _run.last = (o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64))
    return _run.last + (ids, dd, cnt)


def _check(ix, lists, ld, k, drops, id_offset=0, counts=None, what=""):
    gi, gd, gc, ids, dd, cnt = _run(ix, lists, ld, k, drops, id_offset, counts)
    kk = max(k, 1)
    for q in range(len(lists)):
        c = min(int(cnt[q]), ld)
        kept = R.drop_listed(ids[q, :c], np.asarray(drops[q], dtype=np.uint64) + np.uint64(id_offset), k)
        ei = np.zeros(kk, dtype=np.uint64)
        ed = np.zeros(kk, dtype=np.float32)
        ei[:len(kept)] = ids[q, kept]
        ed[:len(kept)] = dd[q, kept]
        if k == 0:
            ei[:], ed[:] = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF), -7.0  # (no slot exists: the sentinel row stays)
        assert gc[q] == len(kept), (what, q, gc[q], len(kept))
        assert np.array_equal(gi[q], ei), (what, q)
        assert gd[q].tobytes() == ed.tobytes(), (what, q)
    return gi, gd, gc


@pytest.mark.parametrize("ld", LDS)
def test_list_lengths_counts_and_k(ix, ld):
    rng = np.random.default_rng(ld)
    for k in sorted({1, max(ld - 1, 1), ld}):
        lists, drops = [], []
        for c in sorted({0, 1, ld // 2, max(ld - 1, 0), ld}):  # counts below ld and ld itself
            rows = rng.permutation(N)[:c]
            for nd in (0, 1, min(c, 5), c):
                lists.append(rows.tolist())
                drops.append(rng.permutation(rows)[:nd].tolist() if nd else [])
            lists.append(rows.tolist())
            drops.append(rng.integers(0, N, size=64).tolist())  # mostly absent ids
        _check(ix, lists, ld, k, drops, what=f"ld={ld} k={k}")


def test_tile_boundaries(ix):
    ld = 200
    rows = list(range(100, 300))
    cases = [
        ([rows[63]], 200), ([rows[64]], 200), ([rows[63], rows[64]], 200), ([rows[0]], 200), ([rows[127], rows[128], rows[199]], 200),
        (rows[:64], 200), (rows[64:128], 200),          # a whole tile listed
        ([rows[5]], 63),                                 # the 63 rows kept of tile 0 fill k: the k-th kept row is lane 63
        ([], 64), ([rows[70]], 127), ([rows[0], rows[1]], 62),
        ([], 128), (rows[1:64], 2),                      # the second kept row is lane 0 of the next tile
    ]
    lists = [rows] * len(cases)
    for k in sorted({c[1] for c in cases}):
        sel = [i for i, c in enumerate(cases) if c[1] == k]
        _check(ix, [lists[i] for i in sel], ld, k, [cases[i][0] for i in sel], what=f"tiles k={k}")


def test_everything_listed_nothing_listed_and_drop_list_sizes(ix):
    rng = np.random.default_rng(9)
    ld = 200
    rows = rng.permutation(N)[:ld].tolist()  # unsorted
    others = [r for r in range(N) if r not in set(rows)]
    for k in (1, 10, 200):
        drops = [rows, [], others[:1024], rows[:1], rows[:64], rows[:65], (rows + others)[:1024], (others + rows)[-1024:], rows[100:] + others[:900]]
        _check(ix, [rows] * len(drops), ld, k, drops, what=f"sizes k={k}")


def test_repeats_in_the_list_and_in_the_drop_list(ix):
    rows = [5, 9, 5, 7, 9, 5, 11, 7, 13] * 10
    drops = [[5], [5, 5], [9, 7, 9], [13, 13, 11, 5, 5], []]
    for k in (1, 4, 90):
        gi, _, gc = _check(ix, [rows] * len(drops), 128, k, drops, what=f"repeats k={k}")
    assert 5 not in gi[0].tolist()[:int(gc[0])] and gc[0] == 60 and gc[4] == 90  # every copy of a listed id goes; repeats otherwise stay


def test_counts_above_ld_and_below_the_list(ix):
    rows = list(range(700, 830))
    _check(ix, [rows[:65]] * 4, 65, 65, [[rows[64]], [rows[3]], [], [rows[0]]], counts=[65, 40, 1000, 0], what="counts")


def test_id_offset(ix):
    rng = np.random.default_rng(12)
    ix.set_id_offset(1 << 33)
    try:
        rows = rng.permutation(N)[:130].tolist()
        _check(ix, [rows] * 3, 130, 100, [rows[::2], [rows[129]], []], id_offset=1 << 33, what="offset")
        # ids are compared as GLOBAL ids: local numbers in the drop list are no rows of the index at all
        with pytest.raises(Exception, match="no row of this index"):
            _run(ix, [rows], 130, 10, [[rows[0]]], id_offset=0)
    finally:
        ix.set_id_offset(0)


def test_refusals_leave_the_outputs_untouched(ix):
    import torch

    import lab_1806_vec_db_amd as vdb

    sent_i, rows = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF), list(range(40))

    def untouched():
        gi, gd, gc = _run.last
        return (gi == sent_i).all() and (gd == -7.0).all() and (gc == sent_i).all()

    with pytest.raises(vdb.VdbError, match="no row of this index"):  # in the list, inside the count
        _run(ix, [rows + [N]], 64, 5, [[1]])
    assert untouched()
    with pytest.raises(vdb.VdbError, match="no row of this index"):  # in the drop list
        _run(ix, [rows, rows], 64, 5, [[1], [2, N + 7]])
    assert untouched()
    _run(ix, [rows + [N]], 64, 5, [[1]], counts=[40])  # beyond the count: not read
    assert _run.last[2][0] == 5
    with pytest.raises(vdb.VdbError, match="at most 1024"):
        _run(ix, [rows], 64, 5, [list(range(1025))])
    assert untouched()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    for lims in ([1, 2], [0, 3, 2]):
        with pytest.raises(vdb.VdbError, match="limits"):
            ix.drop_listed_device(p, p, p, len(lims) - 1, 4, 2, lims, p, p, p, p)
    with pytest.raises(vdb.VdbError, match="null"):
        ix.drop_listed_device(p, p, p, 1, 4, 2, [0, 2], 0, p, p, p)
    with pytest.raises(vdb.VdbError, match="null"):
        ix.drop_listed_device(0, p, p, 1, 4, 2, [0, 0], 0, p, p, p)
    u8 = vdb.GpuIndex(4, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.zeros((8, 4), dtype=np.uint8))
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            u8.drop_listed_device(p, p, p, 1, 4, 2, [0, 0], 0, p, p, p)
    finally:
        u8.close()
    assert not t.cpu().numpy().any()
    # nq == 0 and k == 0: empty results
    ix.drop_listed_device(0, 0, 0, 0, 4, 2, [0], 0, 0, 0, 0)
    gi, gd, gc, *_ = _run(ix, [rows], 64, 0, [[1]])
    assert gc[0] == 0 and (gi == sent_i).all()
