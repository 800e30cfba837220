"""GPU: k_fuse_groups alone (GpuIndex.fuse_groups_device, vdb_fuse_groups_device) over hand-made lists on a 600 x 8 table against
fuse_groups_ref.fuse_groups (verified on the CPU by tests/test_fuse_groups_ref_cpu.py).  The lists are walked as given -- any order of
ids, any distances -- and every comparison is exact: representatives, order, scores as f32 bit patterns, counts, zeros behind the count,
the `exact` byte."""
import threading

import numpy as np
import pytest

import fuse_groups_ref as R
import fuse_ref

pytestmark = pytest.mark.gpu

N = 600
NONE = 0xFFFFFFFF
COL, COL_ROW, COL_WIDE, COL_NEVER = 0, 1, 2, 5
MODES = ("rrf", "min", "sum")
SENT = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)
STATS = ("flat_fused_groups_calls", "flat_fused_groups_queries", "flat_fused_groups_lists", "flat_fused_calls", "flat_grouped_calls",
         "flat_filtered_multi_calls")


@pytest.fixture(scope="module")
def env():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(7)
    ix = vdb.GpuIndex(8, "l2sqr", device=0)
    ix.batch_add(rng.standard_normal((N, 8)).astype(np.float32))
    labels = {}
    c0 = (np.arange(N) // 4).astype(np.uint32)          # 150 documents of 4 chunks
    c0[rng.random(N) < 0.1] = NONE                       # ... a tenth of the rows unlabelled
    labels[COL] = c0
    labels[COL_ROW] = (np.arange(N) * 7 + 3).astype(np.uint32)  # every row a document of its own, through a label
    labels[COL_WIDE] = np.full(N, NONE, dtype=np.uint32)        # written per test through _relabel
    for c in (COL, COL_ROW, COL_WIDE):
        ix.set_labels(c, labels[c])
    labels[COL_NEVER] = None
    yield ix, labels
    ix.close()


def _relabel(env, codes_by_row):
    ix, labels = env
    col = np.full(N, NONE, dtype=np.uint32)
    for r, c in codes_by_row.items():
        col[r] = c
    ix.set_labels(COL_WIDE, col)
    labels[COL_WIDE] = col


def _pack(groups, ld, id_offset=0, counts=None):
    """groups: per fused query a list of lists, each (rows, dists) or rows -> ids [n_lists][ld], dists, counts, lims"""
    flat = [l if isinstance(l, tuple) else (l, None) for g in groups for l in g]
    nl = len(flat)
    ids = np.full((max(nl, 1), max(ld, 1)), 0xDEAD00, dtype=np.uint64)  # (beyond a count: never read -- no row at all)
    dd = np.full((max(nl, 1), max(ld, 1)), -3.0, dtype=np.float32)
    cnt = np.zeros(max(nl, 1), dtype=np.uint64)
    for j, (rows, dists) in enumerate(flat):
        m = len(rows)
        assert m <= ld
        ids[j, :m] = np.asarray(rows, dtype=np.uint64) + np.uint64(id_offset)
        dd[j, :m] = dists if dists is not None else (np.arange(m, dtype=np.float32) * np.float32(0.37) + np.float32(j % 7))
        cnt[j] = m
    if counts is not None:
        cnt[:nl] = np.asarray(counts, dtype=np.uint64)
    lims = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint64)
    return ids, dd, cnt, lims


def _call(ix, ids, dd, cnt, lm, ld, k, mode, column, weights=None, c=60.0, trunc_len=None, want_exact=True):
    import torch

    nq, kk = len(lm) - 1, max(k, 1)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(dd).cuda()
    t_c = torch.from_numpy(cnt.view(np.int64)).cuda()
    o_i = torch.full((max(nq, 1), kk), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((max(nq, 1), kk), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((max(nq, 1),), -7, dtype=torch.int64, device="cuda")
    o_e = torch.full((max(nq, 1),), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.fuse_groups_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), lm, ld, k, column, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(),
                              o_e.data_ptr() if want_exact else 0, mode=mode, weights=weights, rrf_c=c, trunc_len=trunc_len)
    finally:
        torch.cuda.synchronize()
        got = (o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64), o_e.cpu().numpy())
    return got


def _run(ix, groups, ld, k, mode, column, weights=None, c=60.0, id_offset=0, counts=None, lims=None, trunc_len=None, want_exact=True):
    ids, dd, cnt, lm = _pack(groups, ld, id_offset, counts)
    if lims is not None:
        lm = np.asarray(lims, dtype=np.uint64)
    return _call(ix, ids, dd, cnt, lm, ld, k, mode, column, weights, c, trunc_len, want_exact) + (ids, dd, cnt, lm)


def _expected(labels_col, ids, dd, cnt, lm, ld, q, k, mode, weights, c, id_offset, trunc_len):
    lo, hi = int(lm[q]), int(lm[q + 1])
    lists = [(ids[j, :min(int(cnt[j]), ld)], dd[j, :min(int(cnt[j]), ld)]) for j in range(lo, hi)]
    w = None if weights is None else list(weights[lo:hi])
    return R.fuse_groups(lists, R.label_groups(labels_col, id_offset), k, mode, w, c, trunc_len=max(ld, 1) if trunc_len is None else trunc_len)


def _compare(got, exp, k, q, what):
    gi, gd, gc, ge = got
    ei, eb, ec = fuse_ref.padded(exp[0], exp[1], max(k, 1))
    assert gc[q] == ec, (what, q, int(gc[q]), ec)
    assert np.array_equal(gi[q], ei), (what, q, gi[q][:8], ei[:8])
    assert np.array_equal(gd[q].view(np.uint32), eb), (what, q, gd[q][:8], eb.view(np.float32)[:8])
    assert ge[q] == exp[2], (what, q, int(ge[q]), exp[2])


def _check(env, groups, ld, ks, mode, column, weights=None, c=60.0, id_offset=0, counts=None, trunc_len=None, what=""):
    ix, labels = env
    for k in ks:
        gi, gd, gc, ge, ids, dd, cnt, lm = _run(ix, groups, ld, k, mode, column, weights, c, id_offset, counts, None, trunc_len)
        for q in range(len(groups)):
            exp = _expected(labels[column], ids, dd, cnt, lm, ld, q, k, mode, weights, c, id_offset, trunc_len)
            _compare((gi, gd, gc, ge), exp, k, q, f"{what} mode={mode} k={k}")


def _n_groups(labels_col, rows):
    g = R.label_groups(labels_col)
    return len({g(r) for r in rows})


@pytest.mark.parametrize("ld", (1, 63, 64, 65, 255, 256, 257, 513))
def test_list_lengths_list_counts_and_k(env, ld):
    rng = np.random.default_rng(ld)
    _, labels = env
    for S in (1, 2, 5, 32 if 32 * ld <= 16384 else 16384 // ld):
        pool = rng.permutation(N)[:min(N, max(2, (3 * ld) // 2))]  # lists of one fused query overlap in part
        g0 = [rng.permutation(pool)[:ld].tolist() for _ in range(S)]
        g1 = [rng.permutation(pool)[:max(ld - 1, 0)].tolist() for _ in range(S)]
        u = _n_groups(labels[COL], [r for l in g0 for r in l])
        w = rng.uniform(0.5, 2.0, size=2 * S).astype(np.float32)
        for mode in MODES:
            dg = [[(l, np.sort(rng.integers(0, 50, size=len(l))).astype(np.float32) * np.float32(0.25)) for l in g] for g in (g0, g1)]  # ties
            _check(env, dg, ld, (1, u + 5, ld + 3), mode, COL, weights=w if mode == "rrf" else None, what=f"ld={ld} S={S}")


def test_group_across_a_tile_boundary_and_a_late_first_sight(env):
    a = list(range(0, 300))
    _relabel(env, {**{r: 1000 + r for r in range(N)}, a[255]: 77, a[256]: 77, 400: 88, 401: 88})
    # document 77: first occurrence at thread 255 of tile 0, second at thread 0 of tile 1 (and the other way round in list 1)
    l0 = (a, np.arange(300, dtype=np.float32))
    l1 = (a[:255] + [a[256], a[255]] + a[257:], np.arange(300, 0, -1).astype(np.float32))
    # document 88 is first seen in the LAST list only: its sum starts from the fill prefix
    l2 = ([400, 5, 401], np.array([0.5, 0.75, 0.1], dtype=np.float32))
    for mode in MODES:
        _check(env, [[l0, l1, l2], [l0, l2], [l2, l1]], 300, (1, 7, 299, 400), mode, COL_WIDE, c=0.0, what="tile boundary")
    gi, gd, gc, ge, *_ = _run(env[0], [[l0, l1, l2]], 300, 400, "min", COL_WIDE)
    at = gi[0].tolist().index(a[256])            # list 1 holds row 256 at position 255 with distance 45: the smallest of document 77
    assert gd[0][at] == np.float32(45.0) and a[255] not in gi[0, :int(gc[0])].tolist() and gc[0] == 299 + 1  # (299 documents of l0, and 88)


def test_one_label_filling_a_tile_and_a_tile_of_distinct_labels(env):
    rng = np.random.default_rng(3)
    _relabel(env, {r: 9 for r in range(300)})
    rows = rng.permutation(300).tolist()
    for mode in MODES:
        _check(env, [[rows, rows[::-1]], [rows[:256]], [rows[:257], list(range(300, 320))]], 300, (1, 2, 30), mode, COL_WIDE, what="one label")
        _check(env, [[rows, rows[::-1]], [rows[:256], rows[100:290]]], 300, (1, 256, 301), mode, COL_ROW, what="distinct labels")
    gi, gd, gc, ge, *_ = _run(env[0], [[rows, rows[::-1]]], 300, 5, "rrf", COL_WIDE, c=0.0)
    assert gc[0] == 1 and gd[0, 0] == np.float32(2.0)  # one group, rank 0 in both lists


def test_labels_that_collide_in_the_hash_and_the_extreme_codes(env):
    ix, _ = env
    S, ld = 2, 16
    code, s_max, lg, in_lds, _, _ = ix.fuse_groups_plan([0, S], 1, ld, "sum", column=COL_WIDE)
    assert (code, s_max, lg, in_lds) == (0, 2, 6, 1)
    cand = np.arange(1, 200000, dtype=np.uint64)
    h = ((cand * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)  # fuse_groups_hash
    same = cand[h == 17][:16].tolist()                         # 16 codes that all start probing at one slot
    nxt = cand[h == 18][:8].tolist()                           # ... and codes whose own slot the run has taken
    wrap = cand[h == 63][:8].tolist() + cand[h == 0][:8].tolist()  # a run that wraps around the end of the table
    codes = same + nxt + wrap + [0, 0xFFFFFFFE]
    _relabel(env, {r: c for r, c in enumerate(codes)} | {100 + r: c for r, c in enumerate(codes)})  # two rows per code
    r_same, r_nxt, r_wrap, r_ext = list(range(0, 16)), list(range(16, 24)), list(range(24, 40)), [40, 41]
    twin = lambda rows: [100 + r for r in rows]  # noqa: E731
    groups = [[r_same, twin(r_same)[::-1]], [r_same[:8] + r_nxt, twin(r_nxt) + r_same[8:]], [r_wrap, twin(r_wrap)[::-1]],
              [r_ext + r_same[:6], twin(r_ext)[::-1] + r_wrap[:6]], [twin(r_ext) + r_ext]]
    for mode in MODES:
        _check(env, groups, ld, (1, 16, 24, 40), mode, COL_WIDE, what="collide")
    gi, gd, gc, ge, *_ = _run(ix, [[r_ext, twin(r_ext)]], ld, 5, "rrf", COL_WIDE)
    assert gc[0] == 2  # codes 0 and 0xFFFFFFFE: two groups of two rows


def test_unlabelled_rows_that_share_a_number_with_a_label_code(env):
    # rows 5 and 9 are unlabelled; codes 5 and 9 are carried by rows 20 / 21 and 22: four groups, two per number
    _relabel(env, {20: 5, 21: 5, 22: 9, 30: 31, 31: 30})
    groups = [[[5, 20, 9, 22, 21], [21, 9, 5, 22]], [[22, 9], [9, 22]], [[30, 31, 5], [31, 30, 20]]]
    for mode in MODES:
        _check(env, groups, 8, (1, 3, 4, 9), mode, COL_WIDE, c=0.0, what="key spaces")
    gi, gd, gc, ge, *_ = _run(env[0], groups, 8, 9, "rrf", COL_WIDE, c=0.0)
    assert gc.tolist() == [4, 2, 4] and set(gi[1, :2].tolist()) == {9, 22}


def test_a_never_written_column_is_the_row_level_fusion(env):
    import torch

    ix, _ = env
    rng = np.random.default_rng(4)
    groups = [[rng.permutation(N)[:257].tolist() for _ in range(3)], [rng.permutation(N)[:100].tolist() for _ in range(5)]]
    w = rng.uniform(0.5, 2.0, size=8).astype(np.float32)
    for mode in ("rrf", "min"):
        ids, dd, cnt, lm = _pack(groups, 257)
        got = _call(ix, ids, dd, cnt, lm, 257, 50, mode, COL_NEVER, w if mode == "rrf" else None)
        t = [torch.from_numpy(x).cuda() for x in (ids.view(np.int64), dd, cnt.view(np.int64))]
        o_i = torch.zeros((2, 50), dtype=torch.int64, device="cuda")
        o_d = torch.zeros((2, 50), dtype=torch.float32, device="cuda")
        o_c = torch.zeros(2, dtype=torch.int64, device="cuda")
        ix.fuse_lists_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), lm, 257, 50, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode=mode,
                             weights=w if mode == "rrf" else None)
        torch.cuda.synchronize()
        assert np.array_equal(got[0], o_i.cpu().numpy().view(np.uint64)) and np.array_equal(got[2], o_c.cpu().numpy().view(np.uint64))
        assert np.array_equal(got[1].view(np.uint32), o_d.cpu().numpy().view(np.uint32))
    for mode in MODES:
        _check(env, groups, 257, (1, 50, 700), mode, COL_NEVER, what="never written")


def test_special_distances_and_a_nan_as_a_lists_last_entry(env):
    f = lambda u: np.array(u, dtype=np.uint32).view(np.float32)  # noqa: E731
    nan1, nan2 = f(0x7FC00001), f(0xFFC00002)
    _relabel(env, {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 6: 3, 7: 4, 8: 4})
    g = [
        ([1, 3, 5, 7, 10, 11], np.array([nan1, -0.0, 0.0, np.inf, nan1, -np.inf], dtype=np.float32)),
        ([2, 4, 6, 8, 10, 12], np.array([nan2, 0.0, -0.0, -np.inf, 7.0, nan2], dtype=np.float32)),   # ... a NaN as the last entry: the fill
        ([12, 13, 3], np.array([nan1, np.inf, -0.0], dtype=np.float32)),
        ([1, 9], np.array([1e38, 3e38], dtype=np.float32)), ([2, 9], np.array([3e38, 3e38], dtype=np.float32)),  # sums that overflow to +inf
    ]
    groups = [g, g[::-1], [g[1], g[0], g[2]], [g[3], g[4]], [g[0]], [g[4], g[3], g[2]]]
    for mode in MODES:
        _check(env, groups, 6, (1, 3, 8, 12), mode, COL_WIDE, what="special")
    gi, gd, gc, ge, *_ = _run(env[0], [g[:2]], 6, 12, "min", COL_WIDE)
    # documents 4 (-inf), row 11 (-inf), 2 (-0 of list 0), 3 (+0 of list 0), row 10 (7), then the NaNs: document 1 (list 0's bits), row 12
    assert gc[0] == 7 and gi[0, :7].tolist() == [8, 11, 3, 5, 10, 1, 12]
    assert gd[0, :7].view(np.uint32).tolist() == [0xFF800000, 0xFF800000, 0x80000000, 0, 0x40E00000, 0x7FC00001, 0xFFC00002]
    gi, gd, gc, ge, *_ = _run(env[0], [g[:2]], 6, 12, "sum", COL_WIDE)
    # documents 2 and 3 sum their zeros; every other sum meets a NaN (f_1 is one) or inf - inf, and leaves as the one NaN
    assert gc[0] == 7 and gi[0, :2].tolist() == [3, 5] and gd[0, :7].view(np.uint32).tolist() == [0, 0] + [0x7FC00000] * 5


def test_the_same_id_twice_and_short_counts(env):
    rng = np.random.default_rng(11)
    a = rng.permutation(400)[:130].tolist()
    rep = a[:10] + [a[3]] + a[11:20] + [a[3]] + a[21:]
    far = a[:3] + [a[90]] + a[4:]
    for mode in MODES:
        _check(env, [[rep, far], [(rep, np.arange(130, 0, -1).astype(np.float32))]], 130, (1, 50, 200), mode, COL, what="repeats")
        groups = [[rng.permutation(400)[:130].tolist() for _ in range(3)] for _ in range(2)]
        _check(env, groups, 130, (1, 50, 400), mode, COL, counts=[130, 40, 100000, 0, 1, 129], what="counts")


def test_empty_lists_between_full_ones_and_all_lists_empty(env):
    rng = np.random.default_rng(12)
    full = [rng.permutation(N)[:70].tolist() for _ in range(3)]
    groups = [[full[0], [], full[1], [], [], full[2]], [[], full[0]], [full[1], []], [[], [], []], [[]]]
    for mode in MODES:
        _check(env, groups, 70, (1, 40, 300), mode, COL, weights=np.arange(1, 15, dtype=np.float32) if mode == "rrf" else None, what="holes")
        gi, gd, gc, ge, *_ = _run(env[0], groups, 70, 3, mode, COL)
        assert gc.tolist()[3:] == [0, 0] and not gi[3:].any() and not gd[3:].view(np.uint32).any() and ge.tolist()[3:] == [1, 1]
    # ld == 0: every list is empty; k == 0: nothing is ranked
    gi, gd, gc, ge, *_ = _run(env[0], [[[], []], [[]]], 0, 3, "sum", COL)
    assert gc.tolist() == [0, 0] and not gi.any() and not gd.view(np.uint32).any() and ge.tolist() == [1, 1]
    gi, gd, gc, ge, *_ = _run(env[0], [[full[0]]], 70, 0, "sum", COL)
    assert gc[0] == 0 and (gi == SENT).all() and ge[0] == 0


def test_both_table_places_give_the_same_bits(env):
    """32 lists of 60 entries: in a launch of ld = 60 the table (2^12 slots) lives in LDS, in one of ld = 512 (32 x 512 entries: 2^15
    slots) on the scratch buffer; the lists, and so the answers, are the same"""
    ix, _ = env
    rng = np.random.default_rng(13)
    assert ix.fuse_groups_plan([0, 32, 34], 1, 60, "sum")[2:5] == (12, 1, 0)
    assert ix.fuse_groups_plan([0, 32, 34], 1, 512, "sum")[2:5] == (15, 0, 28 << 15)
    assert ix.fuse_groups_plan([0, 2], 1, 1024, "sum")[2:4] == (12, 1) and ix.fuse_groups_plan([0, 2], 1, 1025, "sum")[2:4] == (13, 0)
    g0 = [(rng.permutation(N)[:60].tolist(), np.sort(rng.integers(0, 90, size=60)).astype(np.float32)) for _ in range(32)]
    g1 = [(rng.permutation(N)[:60].tolist(), np.sort(rng.integers(0, 90, size=60)).astype(np.float32)) for _ in range(2)]  # a second slice
    w = rng.uniform(0.5, 2.0, size=34).astype(np.float32)
    for mode in MODES:
        for column in (COL, COL_ROW):
            ww = w if mode == "rrf" else None
            a = _run(ix, [g0, g1], 60, 150, mode, column, ww, trunc_len=60)[:4]
            b = _run(ix, [g0, g1], 512, 150, mode, column, ww, trunc_len=60)[:4]
            assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b)), (mode, column)
        _check(env, [g0, g1], 512, (1, 150, 600), mode, COL, weights=w if mode == "rrf" else None, trunc_len=60, what="scratch")
    # lists that fill the scratch table: 32 x 512 entries over all 600 rows, and 2 x 1025: the first length past LDS
    big = [[rng.permutation(N)[:512].tolist() for _ in range(32)]]
    for mode in MODES:
        _check(env, big, 512, (10, 600), mode, COL_ROW, what="32 x 512")
    long = [[np.concatenate([rng.permutation(N), rng.permutation(N)])[:1025].tolist() for _ in range(2)]]
    for mode in MODES:
        _check(env, long, 1025, (10, 1100), mode, COL, what="2 x 1025")


def test_one_list_under_min_is_the_capped_walk_at_group_size_one(env):
    import torch

    ix, _ = env
    rng = np.random.default_rng(14)
    rows = [rng.permutation(N)[:300] for _ in range(3)]
    dists = [np.sort(rng.integers(0, 40, size=300)).astype(np.float32) for _ in range(3)]  # sorted, with ties
    for q in range(3):  # ... ties in (distance, id) order, as a search returns them
        o = np.lexsort((rows[q], dists[q]))
        rows[q] = rows[q][o]
    groups = [[(rows[q].tolist(), dists[q])] for q in range(3)]
    for k in (1, 20, 400):
        gi, gd, gc, ge, ids, dd, cnt, lm = _run(ix, groups, 300, k, "min", COL)
        t = [torch.from_numpy(x).cuda() for x in (ids.view(np.int64), dd, cnt.view(np.int64))]
        o_i = torch.zeros((3, k), dtype=torch.int64, device="cuda")
        o_d = torch.zeros((3, k), dtype=torch.float32, device="cuda")
        o_c = torch.zeros(3, dtype=torch.int64, device="cuda")
        ix.group_cap_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 3, 300, k, COL, 1, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(gc, o_c.cpu().numpy().view(np.uint64)), k
        assert np.array_equal(gi, o_i.cpu().numpy().view(np.uint64)) and np.array_equal(gd.view(np.uint32), o_d.cpu().numpy().view(np.uint32)), k


def test_out_exact_in_every_branch(env):
    ix, _ = env
    _relabel(env, {0: 1, 1: 1, 3: 2, 4: 2, 5: 3, 8: 4, 9: 4})
    lists = [[([0, 3], np.array([1.0, 2.0], dtype=np.float32)), ([5], np.array([1.5], dtype=np.float32))]]
    ex = lambda k, mode, tl: int(_run(ix, lists, 2, k, mode, COL_WIDE, trunc_len=tl)[3][0])  # noqa: E731
    assert [ex(1, "min", 2), ex(2, "min", 2), ex(3, "min", 2), ex(4, "min", 2), ex(4, "min", 3)] == [1, 1, 0, 0, 1]  # a tie AT f_0 gives 0
    assert [ex(1, "rrf", 2), ex(1, "sum", 2), ex(1, "rrf", 3), ex(1, "sum", 3), ex(1, "sum", None)] == [0, 0, 1, 1, 0]
    two = [[([0, 3], np.array([1.0, 2.0], dtype=np.float32)), ([5, 8], np.array([0.5, 1.0], dtype=np.float32))]]
    assert [int(_run(ix, two, 2, k, "min", COL_WIDE)[3][0]) for k in (1, 2)] == [1, 0]  # the smaller f decides
    assert int(_run(ix, [[([0, 3], np.array([-0.0, 0.0], dtype=np.float32))]], 2, 1, "min", COL_WIDE)[3][0]) == 0  # -0 == +0: a tie
    # a NULL out_exact is not written and changes nothing else
    a, b = _run(ix, two, 2, 3, "min", COL_WIDE), _run(ix, two, 2, 3, "min", COL_WIDE, want_exact=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and b[3][0] == 77
    # per fused query, and on the scratch table
    rng = np.random.default_rng(15)
    g = [[(rng.permutation(N)[:int(m)].tolist(), np.sort(rng.integers(0, 30, size=int(m))).astype(np.float32)) for m in rng.integers(1, 65, size=4)]
         for _ in range(12)]
    for mode in MODES:
        _check(env, g, 64, (1, 5, 60), mode, COL, trunc_len=40, what="exact")
        _check(env, g[:3], 4096, (5,), mode, COL, trunc_len=40, what="exact, scratch")


def test_id_offset(env):
    import lab_1806_vec_db_amd as vdb

    ix, _ = env
    rng = np.random.default_rng(16)
    off = (1 << 33) + 5
    ix.set_id_offset(off)
    try:
        groups = [[rng.permutation(N)[:100].tolist() for _ in range(3)], [[N - 1, 0], [0, N - 1]]]
        for mode in MODES:
            _check(env, groups, 100, (1, 30, 300), mode, COL, id_offset=off, what="offset")
        assert _run(ix, groups, 100, 5, "min", COL, id_offset=off)[0][0].min() >= off
        with pytest.raises(vdb.VdbError, match="no row of this index"):  # local numbers are no rows of the index now
            _run(ix, groups, 100, 5, "rrf", COL, id_offset=0)
    finally:
        ix.set_id_offset(0)


def test_refusals_leave_outputs_and_counters_untouched(env):
    import torch

    import lab_1806_vec_db_amd as vdb

    ix, _ = env
    rows = list(range(40))
    before = {s: ix.get_stat(s) for s in STATS}

    def refused(match, groups, ld, k, mode, column=COL, **kw):
        ids, dd, cnt, lm = _pack(groups, ld, counts=kw.pop("counts", None))
        if "lims" in kw:
            lm = np.asarray(kw.pop("lims"), dtype=np.uint64)
        nq, kk = len(lm) - 1, max(k, 1)
        t = [torch.from_numpy(x).cuda() for x in (ids.view(np.int64), dd, cnt.view(np.int64))]
        o_i = torch.full((max(nq, 1), kk), -7, dtype=torch.int64, device="cuda")
        o_d = torch.full((max(nq, 1), kk), -7.0, dtype=torch.float32, device="cuda")
        o_c = torch.full((max(nq, 1),), -7, dtype=torch.int64, device="cuda")
        o_e = torch.full((max(nq, 1),), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(vdb.VdbError, match=match):
            ix.fuse_groups_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), lm, ld, k, column, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(),
                                  o_e.data_ptr(), mode=mode, **kw)
        torch.cuda.synchronize()
        assert (o_i.cpu().numpy() == -7).all() and (o_d.cpu().numpy() == -7.0).all() and (o_c.cpu().numpy() == -7).all(), match
        assert (o_e.cpu().numpy() == 77).all(), match

    refused("no row of this index", [[rows, rows + [N]]], 64, 5, "rrf")       # inside the count
    refused("no row of this index", [[rows], [[N + 9]]], 64, 5, "sum")
    assert _run(ix, [[rows + [N]]], 64, 5, "sum", COL, counts=[40])[2][0] == 5  # beyond the count: not read
    refused("mode", [[rows]], 64, 5, 3)
    refused("start at 0", [[rows]], 64, 5, "sum", lims=[1, 1])
    refused("not decrease", [[rows], [rows]], 64, 5, "sum", lims=[0, 2, 1])
    refused("at least one sub-query", [[rows], [rows]], 64, 5, "sum", lims=[0, 0, 2])
    refused("at most 32", [[rows] * 33], 64, 5, "sum")
    refused("at most 4096", [[rows]], 4097, 5, "sum")
    refused("at most 16384", [[rows] * 5], 4096, 5, "sum")
    refused("at most 16384", [[rows] * 17], 1024, 5, "min")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("weight", [[rows, rows]], 64, 5, "rrf", weights=[1.0, bad])
    refused("VDB_FUSE_RRF only", [[rows]], 64, 5, "min", weights=[1.0])
    refused("no weighted VDB_FUSE_SUM", [[rows]], 64, 5, "sum", weights=[1.0])
    for bad in (-1.0, float("nan"), float("inf")):
        refused("rrf_c", [[rows]], 64, 5, "sum", rrf_c=bad)
    refused("VDB_LABEL_COLUMNS", [[rows]], 64, 5, "sum", column=16)
    refused("trunc_len", [[rows]], 64, 5, "sum", trunc_len=0)
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    with pytest.raises(vdb.VdbError, match="null"):
        ix.fuse_groups_device(0, p, p, [0, 1], 4, 2, COL, p, p, p)
    with pytest.raises(ValueError, match="fusion mode"):
        ix.fuse_groups_device(p, p, p, [0, 1], 4, 2, COL, p, p, p, mode="max")
    u8 = vdb.GpuIndex(4, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.zeros((8, 4), dtype=np.uint8))
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            u8.fuse_groups_device(p, p, p, [0, 1], 4, 2, COL, p, p, p)
    finally:
        u8.close()
    assert not t.cpu().numpy().any()
    ix.fuse_groups_device(0, 0, 0, [0], 4, 2, COL, 0, 0, 0)  # nq == 0
    assert {s: ix.get_stat(s) for s in STATS} == before  # the list form counts nothing, refused or not


def test_two_threads(env):
    ix, labels = env
    rng = np.random.default_rng(21)
    jobs = []
    for t in range(2):
        groups = [[rng.permutation(N)[:257].tolist() for _ in range(3 + t)] for _ in range(20)]
        jobs.append((groups, "rrf" if t == 0 else "sum"))
    out, err = [None, None], []

    def work(t):
        try:
            for _ in range(5):
                ids, dd, cnt, lm = _pack(jobs[t][0], 257)
                out[t] = _call(ix, ids, dd, cnt, lm, 257, 50, jobs[t][1], COL) + (ids, dd, cnt, lm)
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for t in range(2):
        gi, gd, gc, ge, ids, dd, cnt, lm = out[t]
        for q in range(20):
            exp = _expected(labels[COL], ids, dd, cnt, lm, 257, q, 50, jobs[t][1], None, 60.0, 0, None)
            _compare((gi, gd, gc, ge), exp, 50, q, f"thread {t}")
