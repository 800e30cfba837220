"""GPU: k_group_cap alone (GpuIndex.group_cap_device, vdb_group_cap_device) over hand-made candidate lists against labels.cap_groups, the
host statement of the walk.  The lists are walked as given -- any order of ids, any distances -- so the expected answer of a query is
cap_groups over the labels of its ids: the kept (id, distance) pairs in list order, zeros behind them, their count.  Everything is
compared exactly (distances as f32 bit patterns: the kernel only moves them)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 6000
NONE = 0xFFFFFFFF
COL, COL_MANY, COL_WIDE, COL_NEVER = 0, 1, 2, 5


def _table_lg(k, ld):  # grouped_plan.hpp: grouped_table_lg (tests/test_grouped_plan_cpu.py checks the header against this)
    need, lg = 2 * (min(k, ld) + 64), 7
    while (1 << lg) < need:
        lg += 1
    return lg


def _hash(label, lg):  # grouped_plan.hpp: grouped_hash
    return ((label * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


@pytest.fixture(scope="module")
def env():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(77)
    ix = vdb.GpuIndex(4, "l2sqr", device=0)
    ix.batch_add(rng.random((N, 4), dtype=np.float32))
    labels = {}
    # column 0: six values, one of them on 40 % of the rows (so that g = 64 and 65 still cap within 1000 positions), a tenth unlabelled
    c0 = rng.choice(np.array([3, 4, 5, 6, 7, 0xFFFFFFFE, NONE], dtype=np.uint32), size=N, p=[0.4, 0.2, 0.1, 0.1, 0.05, 0.05, 0.1])
    labels[COL] = c0
    labels[COL_MANY] = (np.arange(N) % 2500).astype(np.uint32)  # 2500 values: enough kept rows for a k past the LDS table
    # column 2: written per test through `relabel`
    labels[COL_WIDE] = np.full(N, NONE, dtype=np.uint32)
    for c in (COL, COL_MANY, COL_WIDE):
        ix.set_labels(c, labels[c])
    labels[COL_NEVER] = np.full(N, NONE, dtype=np.uint32)
    yield ix, labels, rng
    ix.close()


def _relabel(env, codes_by_row):
    ix, labels, _ = env
    col = np.full(N, NONE, dtype=np.uint32)
    for r, c in codes_by_row.items():
        col[r] = c
    ix.set_labels(COL_WIDE, col)
    labels[COL_WIDE] = col


def _run(ix, lists, ld, k, column, g, id_offset=0, counts=None):
    """lists: per query an array of LOCAL rows; -> (idx, dist, cnt) from the device, outputs pre-filled with a sentinel; also the distances used"""
    import torch

    nq = len(lists)
    ids = np.full((nq, max(ld, 1)), 0xDEAD, dtype=np.uint64)  # (beyond a count: never read -- 0xDEAD + offset may be no row at all)
    dists = np.zeros((nq, max(ld, 1)), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q, rows in enumerate(lists):
        ids[q, :len(rows)] = np.asarray(rows, dtype=np.uint64) + np.uint64(id_offset)
        dists[q, :len(rows)] = (np.arange(len(rows)) * 0.37 + q).astype(np.float32)
        cnt[q] = len(rows)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.uint64)
    kk = max(k, 1)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(dists).cuda()
    t_c = torch.from_numpy(cnt.view(np.int64)).cuda()
    o_i = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.group_cap_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), nq, ld, k, column, g, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())
    finally:
        torch.cuda.synchronize()
        got = (o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64))
        _run.last = got
    return got, dists


def _expect(labels_col, lists, dists, k, g, id_offset=0):
    from lab_1806_vec_db_amd.labels import cap_groups

    nq, kk = len(lists), max(k, 1)
    idx = np.zeros((nq, kk), dtype=np.uint64)
    dist = np.zeros((nq, kk), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q, rows in enumerate(lists):
        rows = np.asarray(rows, dtype=np.int64)
        kept = cap_groups(labels_col[rows], g, k)
        cnt[q] = len(kept)
        idx[q, :len(kept)] = rows[kept].astype(np.uint64) + np.uint64(id_offset)
        dist[q, :len(kept)] = dists[q, kept]
    if k == 0:
        idx[:], dist[:] = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF), -7.0  # (nothing is written for k = 0)
    return idx, dist, cnt


def _check(env, lists, ld, k, column, g, id_offset=0, what=""):
    ix, labels, _ = env
    (gi, gd, gc), dists = _run(ix, lists, ld, k, column, g, id_offset)
    ei, ed, ec = _expect(labels[column], lists, dists, k, g, id_offset)
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei), what
    assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), what
    return gi, gd, gc


LENGTHS = (0, 1, 63, 64, 65, 128, 129, 1000)


@pytest.mark.parametrize("g", (1, 2, 3, 64, 65))
def test_lengths_and_group_sizes(env, g):
    """every list length around the tile size in ONE call (so the counts differ within it), k below, at and above what the walk keeps"""
    rng = env[2]
    lists = [rng.choice(N, size=n, replace=False) for n in LENGTHS]
    for k in (1, 10, 1000):
        _, _, gc = _check(env, lists, 1000, k, COL, g, what=(g, k))
    assert gc[-1] < 1000 and gc[0] == 0  # (the cap bit in the longest list; the empty list kept nothing)


@pytest.mark.parametrize("g", (1, 2, 3, 64))
def test_gth_occurrence_at_the_tile_boundary(env, g):
    """one label across a tile boundary: its g-th occurrence at lane 63 of tile 0 (kept) and the next at lane 0 of tile 1 (dropped); and
    the g-th at lane 0 of tile 1 (kept), the next at lane 1 (dropped)"""
    rows = np.arange(200, 200 + 192)
    for last_kept in (63, 64):
        pos = list(range(last_kept - (g - 1), last_kept + 1)) + [last_kept + 1, 100, 191]  # g occurrences ending at last_kept, then three more
        _relabel(env, {int(rows[p]): 42 for p in pos} | {int(rows[p]): 1000 + p for p in range(192) if p not in pos and p % 3})
        gi, _, gc = _check(env, [rows], 192, 192, COL_WIDE, g, what=(g, last_kept))
        kept = set(gi[0, :int(gc[0])].tolist())
        assert int(rows[last_kept]) in kept and int(rows[last_kept + 1]) not in kept and int(rows[100]) not in kept and int(rows[191]) not in kept
        assert int(gc[0]) == 192 - 3


def test_distinct_labels_and_one_label_filling_a_tile(env):
    rows = np.arange(1000, 1000 + 200)
    _relabel(env, {int(r): 5000 + i for i, r in enumerate(rows)})  # 64 distinct labels in every tile
    for g in (1, 2):
        _, _, gc = _check(env, [rows, rows[:64], rows[:65]], 200, 200, COL_WIDE, g)
        assert gc.tolist() == [200, 64, 65]
    _relabel(env, {int(r): 9 for r in rows})  # one label fills every tile
    for g, want in ((1, 1), (2, 2), (63, 63), (64, 64), (65, 65), (1000, 200)):
        _, _, gc = _check(env, [rows], 200, 200, COL_WIDE, g)
        assert int(gc[0]) == want


def test_hash_collisions_and_large_codes(env):
    """labels that start probing at the same slot of the walk's table, and labels a multiple of the capacity apart, up to 0xFFFFFFFE"""
    ld = k = 300
    lg = _table_lg(k, ld)
    cap = 1 << lg
    same_slot = [c for c in range(1, 400000) if _hash(c, lg) == _hash(1, lg)][:40]
    assert len(same_slot) == 40
    apart = [7 + i * cap for i in range(40)] + [0xFFFFFFFE - i * cap for i in range(40)]
    codes = same_slot + apart
    rows = np.arange(2000, 2000 + ld)
    rng = env[2]
    _relabel(env, {int(r): int(codes[int(rng.integers(len(codes)))]) for r in rows})
    for g in (1, 2, 3):
        _check(env, [rows, rows[::-1], rows[:129]], ld, k, COL_WIDE, g, what=g)
    _check(env, [rows], ld, 5, COL_WIDE, 1)  # (a smaller table: other collisions)


def test_unlabelled_rows_are_never_capped(env):
    ix, labels, rng = env
    rows = np.arange(3000, 3000 + 300)
    _relabel(env, {int(r): 11 for r in rows[::2]})  # every second row labelled with ONE value, the others unlabelled
    _, _, gc = _check(env, [rows], 300, 300, COL_WIDE, 1)
    assert int(gc[0]) == 151
    # a never-written column: the list itself, cut at k
    lists = [rng.choice(N, size=n, replace=False) for n in (5, 64, 700)]
    for k in (1, 64, 700):
        gi, _, gc = _check(env, lists, 700, k, COL_NEVER, 1)
        assert gc.tolist() == [min(k, 5), min(k, 64), min(k, 700)]
    assert ix.get_stat("label_columns") == 3


def test_k_edges_and_the_global_table(env):
    ix, labels, rng = env
    from lab_1806_vec_db_amd.labels import cap_groups

    rows = rng.choice(N, size=5000, replace=False)
    total = len(cap_groups(labels[COL_MANY][rows], 2, 10**9))
    assert total > 3100
    for k in (1, total, total + 9, 3000):  # (3000: 2 x (3000 + 64) slots are 2^13 -- past the LDS table, see test_grouped_plan_cpu)
        assert (_table_lg(k, 5000) > 12) == (k >= 1985)
        _, _, gc = _check(env, [rows, rows[:100]], 5000, k, COL_MANY, 2, what=k)
        assert int(gc[0]) == min(k, total)
    _check(env, [rows[:10]], 10, 0, COL_MANY, 2)  # k = 0: nothing written but the count


def test_counts_are_clipped_and_differ(env):
    """a count above ld reads ld entries; entries past a count are not read (they hold ids of no row)"""
    ix, labels, rng = env
    lists = [rng.choice(N, size=n, replace=False) for n in (70, 70, 3)]
    (gi, gd, gc), dists = _run(ix, lists, 70, 70, COL, 1, counts=[1000, 70, 3])
    ei, ed, ec = _expect(labels[COL], lists, dists, 70, 1)
    assert np.array_equal(gc, ec) and np.array_equal(gi, ei) and np.array_equal(gd, ed)


def test_id_offset(env):
    ix, labels, rng = env
    ix.set_id_offset(1 << 33)
    try:
        lists = [rng.choice(N, size=n, replace=False) for n in (129, 64)]
        gi, _, gc = _check(env, lists, 129, 100, COL, 2, id_offset=1 << 33)
        assert (gi[0, :int(gc[0])] >= np.uint64(1 << 33)).all()
    finally:
        ix.set_id_offset(0)


def test_out_of_range_id_is_refused(env):
    import lab_1806_vec_db_amd as vdb

    ix, labels, rng = env
    before = {s: ix.get_stat(s) for s in ("flat_grouped_calls", "flat_grouped_queries", "flat_grouped_rounds")}
    for bad, off in ((N, 0), (1 << 40, 0), (5, 1000)):  # the first id past the rows; far past; below id_offset
        ix.set_id_offset(off)
        try:
            lists = [np.arange(10) + off, np.array([1 + off, 2 + off, bad, 3 + off])]  # (the ids as passed: id_offset included)
            with pytest.raises(vdb.VdbError):
                _run(ix, lists, 10, 5, COL, 1)
            gi, gd, gc = _run.last
            assert (gi == np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)).all() and (gd == -7.0).all() and (gc == np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)).all()
        finally:
            ix.set_id_offset(0)
    for g, col in ((0, COL), (1, 16)):
        with pytest.raises(vdb.VdbError):
            _run(ix, [np.arange(4)], 4, 2, col, g)
        assert (_run.last[0] == np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)).all()
    assert before == {s: ix.get_stat(s) for s in before}
    _check(env, [np.arange(10)], 10, 5, COL, 1)  # the index still answers


def test_bad_id_text_and_the_call_after_it():
    """64 rows x dim 8, lists [2][4] with an id equal to len + id_offset, an id below id_offset, and both: the call raises with the exact
    text, the outputs keep their sentinel, and the valid call that follows on the same index is answered -- the flag word of the id check
    is zeroed by every call"""
    import re

    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(6)
    ix = vdb.GpuIndex(8, "l2sqr", device=0)
    try:
        ix.batch_add(rng.random((64, 8), dtype=np.float32))
        col = (np.arange(64) % 2).astype(np.uint32)
        ix.set_labels(COL, col)
        off = 1000
        ix.set_id_offset(off)
        good = [np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7])]
        text = "group cap: a list holds an id that is no row of this index (id - id_offset must be below len)"
        sent = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)
        for past, below in ((True, False), (False, True), (True, True)):
            lists = [g + off for g in good]  # (the ids as passed: id_offset included)
            if past:
                lists[0][2] = 64 + off
            if below:
                lists[1][1] = off - 1
            with pytest.raises(vdb.VdbError, match=re.escape(text)):
                _run(ix, lists, 4, 3, COL, 1)
            assert (_run.last[0] == sent).all() and (_run.last[1] == -7.0).all() and (_run.last[2] == sent).all()
            _, _, gc = _check((ix, {COL: col}, rng), good, 4, 3, COL, 1, id_offset=off, what=("after", past, below))
            assert gc.tolist() == [2, 2]  # (one row per label value: two values in every list)
    finally:
        ix.close()
