"""GPU: k_fuse_lists alone (GpuIndex.fuse_lists_device, vdb_fuse_lists_device) over hand-made lists on a 1500 x 4 table against
fuse_ref.fuse (verified on the CPU by tests/test_fuse_ref_cpu.py).  The lists are walked as given -- any order of ids, any distances --
and every comparison is exact: ids, order, scores as f32 bit patterns, counts, zeros behind the count."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_ref as R

pytestmark = pytest.mark.gpu

N = 1500
LDS = (1, 63, 64, 65, 255, 256, 257, 1024)
SENT = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)
STATS = ("flat_fused_calls", "flat_fused_queries", "flat_fused_lists", "flat_mmr_calls", "flat_grouped_calls", "flat_filtered_multi_calls")


@pytest.fixture(scope="module")
def ix():
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(4, "l2sqr", device=0)
    ix.batch_add(np.random.default_rng(1).standard_normal((N, 4)).astype(np.float32))
    yield ix
    ix.close()


def _plan(lims, k, fetch_k, mode=0, weights=None, c=60.0, budget=0):
    """vdb_fuse_plan -> (code, s_max, lg, in_lds, scratch bytes, sub-chunk)"""
    from lab_1806_vec_db_amd import _lib as L

    so = L.load()
    lm = np.asarray(lims, dtype=np.uint64)
    w = None if weights is None else np.asarray(weights, dtype=np.float32)
    code, in_lds, lg = C.c_int(-1), C.c_int(-1), C.c_uint32(0)
    s_max, scratch, sub = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    st = so.vdb_fuse_plan(mode, lm.ctypes.data_as(L.u64p), len(lm) - 1, k, fetch_k, None if w is None else w.ctypes.data_as(L.f32p), c, budget,
                          C.byref(code), C.byref(s_max), C.byref(lg), C.byref(in_lds), C.byref(scratch), C.byref(sub))
    assert st == 0
    return code.value, s_max.value, lg.value, in_lds.value, scratch.value, sub.value


def _pack(groups, ld, id_offset=0, counts=None):
    """groups: per fused query a list of lists, each (rows, dists) or rows -> ids [n_lists][ld], dists, counts, lims and the flat lists"""
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


def _run(ix, groups, ld, k, mode, weights=None, c=60.0, id_offset=0, counts=None, lims=None):
    import torch

    ids, dd, cnt, lm = _pack(groups, ld, id_offset, counts)
    if lims is not None:
        lm = np.asarray(lims, dtype=np.uint64)
    nq, kk = len(lm) - 1, max(k, 1)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(dd).cuda()
    t_c = torch.from_numpy(cnt.view(np.int64)).cuda()
    o_i = torch.full((max(nq, 1), kk), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((max(nq, 1), kk), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((max(nq, 1),), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    last = None
    try:
        ix.fuse_lists_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), lm, ld, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode=mode,
                             weights=weights, rrf_c=c)
    finally:
        torch.cuda.synchronize()
        last = (o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64))
        _run.last = last
    return last + (ids, dd, cnt, lm)


def _expected(ids, dd, cnt, lm, ld, q, mode, weights, c):
    """the full fused ranking of fused query q (k = everything): a prefix of it answers every k"""
    lo, hi = int(lm[q]), int(lm[q + 1])
    lists = [(ids[j, :min(int(cnt[j]), ld)], dd[j, :min(int(cnt[j]), ld)]) for j in range(lo, hi)]
    w = None if weights is None else list(weights[lo:hi])
    return R.fuse(lists, 1 << 30, mode, w, c)


def _compare(got, exp, k, q, what):
    gi, gd, gc = got
    ei, eb, ec = R.padded(exp[0][:k], exp[1][:k], max(k, 1))
    assert gc[q] == ec, (what, q, int(gc[q]), ec)
    assert np.array_equal(gi[q], ei), (what, q, gi[q][:8], ei[:8])
    assert np.array_equal(gd[q].view(np.uint32), eb), (what, q, gd[q][:8], eb.view(np.float32)[:8])


def _check(ix, groups, ld, ks, mode, weights=None, c=60.0, id_offset=0, counts=None, what=""):
    """one reference per fused query, one device call per k"""
    exp = None
    for k in ks:
        gi, gd, gc, ids, dd, cnt, lm = _run(ix, groups, ld, k, mode, weights, c, id_offset, counts)
        if exp is None:
            exp = [_expected(ids, dd, cnt, lm, ld, q, mode, weights, c) for q in range(len(groups))]
        for q in range(len(groups)):
            _compare((gi, gd, gc), exp[q], k, q, f"{what} mode={mode} k={k}")
    return exp


def _ks(u):
    return sorted({1, 2, max(u - 1, 1), max(u, 1), u + 5})


@pytest.mark.parametrize("ld", LDS)
def test_list_lengths_list_counts_and_k(ix, ld):
    rng = np.random.default_rng(ld)
    for S in (1, 2, 3, 32 if 32 * ld <= 16384 else 16384 // ld):
        pool = rng.permutation(N)[:min(N, max(2, (3 * ld) // 2))]  # lists of one fused query overlap in part
        g0 = [rng.permutation(pool)[:ld].tolist() for _ in range(S)]
        g1 = [rng.permutation(pool)[:max(ld - 1, 0)].tolist() for _ in range(S)]
        u = len({r for l in g0 for r in l})
        w = rng.uniform(0.5, 2.0, size=2 * S).astype(np.float32)
        _check(ix, [g0, g1], ld, _ks(u), "rrf", weights=w, what=f"ld={ld} S={S}")
        dg = [[(l, rng.integers(0, 50, size=len(l)).astype(np.float32) * np.float32(0.25)) for l in g] for g in (g0, g1)]  # ties across lists
        _check(ix, dg, ld, _ks(u), "min", what=f"ld={ld} S={S}")


@pytest.mark.parametrize("nq", (1, 2, 257))
def test_ragged_fused_queries(ix, nq):
    rng = np.random.default_rng(nq)
    groups = []
    for q in range(nq):
        S = 1 + (q * 7) % 5
        groups.append([rng.integers(0, 200, size=int(rng.integers(0, 66))).tolist() for _ in range(S)])  # repeats and empty lists included
    for mode in ("rrf", "min"):
        _check(ix, groups, 65, (1, 10, 300), mode, what=f"ragged nq={nq}")


def test_overlap_patterns_tile_boundaries_and_repeats(ix):
    a = list(range(0, 300))
    b = list(range(300, 600))
    shared = 999
    tile_a = a[:255] + [shared] + a[256:]          # the shared row at the last lane of tile 0 ...
    tile_b = b[:256] + [shared] + b[257:]          # ... and at the first lane of tile 1
    rep_in = a[:10] + [a[3]] + a[11:20] + [a[3]] + a[21:]           # the same id twice more inside one tile
    rep_x = a[:255] + [a[255], a[255]] + a[257:]                    # ... at positions 255 and 256: across two tiles
    rep_far = a[:3] + [shared] + a[4:290] + [shared] + a[291:]      # ... at positions 3 and 290
    groups = [[a, b], [a, a, a], [tile_a, tile_b], [rep_in, b], [rep_x, rep_x], [rep_far, tile_b], [a[::-1], a]]
    for mode in ("rrf", "min"):
        dg = groups
        if mode == "min":  # descending distances: a later occurrence of a repeat has the smaller distance and must still not count
            dg = [[(l, np.arange(len(l), 0, -1).astype(np.float32)) for l in g] for g in groups]
        exp = _check(ix, dg, 300, (1, 7, 300, 650), mode, c=0.0, what="overlap")
        assert len(exp[0][0]) == 600 and len(exp[1][0]) == 300 and len(exp[2][0]) == 599
    # the repeat's first occurrence decides: under MIN row a[3] keeps the distance of position 3, not the smaller ones behind it
    gi, gd, gc, *_ = _run(ix, [[(rep_in, np.arange(300, 0, -1).astype(np.float32))]], 300, 300, "min")
    assert gc[0] == 298 and gd[0][gi[0].tolist().index(a[3])] == np.float32(297.0)


def test_all_equal_scores_come_in_id_order(ix):
    rows = np.random.default_rng(3).permutation(N)[:32].tolist()
    g = [[r] for r in rows]  # 32 lists of one row each: every score is 1 / (1 + c)
    gi, gd, gc, *_ = _run(ix, [g], 1, 40, "rrf")
    assert gc[0] == 32 and gi[0, :32].tolist() == sorted(rows) and len(set(gd[0, :32].view(np.uint32).tolist())) == 1
    _check(ix, [g], 1, (1, 31, 32, 37), "rrf", what="equal")
    _check(ix, [[(rows, np.full(32, 2.5, dtype=np.float32))], [([r], [1.0]) for r in rows]], 32, (5, 32, 40), "min", what="equal")


def test_ids_that_collide_in_the_tables_hash(ix):
    S, ld = 2, 16
    code, s_max, lg, in_lds, _, _ = _plan([0, S], 1, ld)
    assert (code, s_max, lg, in_lds) == (0, 2, 6, 1)
    h = ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)  # fuse_hash
    buckets = [np.flatnonzero(h == b) for b in range(1 << lg)]
    big = max(range(1 << lg), key=lambda b: len(buckets[b]))
    assert len(buckets[big]) >= 16
    same = buckets[big][:16].tolist()                       # 16 rows that all start probing at one slot
    nxt = buckets[(big + 1) % (1 << lg)][:8].tolist()       # ... and rows whose own slot the run has taken
    last = buckets[(1 << lg) - 1][:8].tolist() + buckets[0][:8].tolist()  # a run that wraps around the end of the table
    groups = [[same, same[::-1]], [same[:8] + nxt, nxt + same[8:]], [last, last[::-1]], [same, nxt + last[:8]]]
    for mode in ("rrf", "min"):
        _check(ix, groups, ld, (1, 16, 24, 40), mode, what="collide")


@pytest.mark.parametrize("c", (0.0, 1.0, 60.0))
def test_weights_and_c(ix, c):
    rng = np.random.default_rng(int(c) + 40)
    groups = [[rng.permutation(120)[:64].tolist() for _ in range(S)] for S in (1, 4, 8, 3)]
    w = np.float32(10.0) ** rng.uniform(-3, 3, size=16).astype(np.float32)
    w[:3] = (1e-3, 1e3, 1.0)
    _check(ix, groups, 64, (1, 10, 120), "rrf", weights=w, c=c, what=f"weights c={c}")
    _check(ix, groups, 64, (10,), "rrf", weights=None, c=c, what=f"unweighted c={c}")
    _check(ix, [[[5], [5], [5]], [[5], [5], [5]]], 1, (1,), "rrf", weights=np.array([1e8, 3, 3, 3, 3, 1e8], dtype=np.float32), c=0.0, what="fold order")
    gd = _run.last[1].view(np.uint32)
    assert gd[0, 0] != gd[1, 0]  # (1e8 + 3) + 3 against (3 + 3) + 1e8: the fold runs in list order


def test_min_with_nan_inf_and_signed_zero(ix):
    f = lambda u: np.array(u, dtype=np.uint32).view(np.float32)  # noqa: E731
    nan1, nan2 = f(0x7FC00001), f(0xFFC00002)
    g = [
        ([1, 2, 3, 4, 5, 7], np.array([nan1, -0.0, 0.0, np.inf, nan1, -np.inf], dtype=np.float32)),
        ([1, 2, 3, 4, 5, 6], np.array([nan2, 0.0, -0.0, -np.inf, 7.0, nan2], dtype=np.float32)),
        ([6, 8, 2], np.array([nan1, np.inf, -0.0], dtype=np.float32)),
    ]
    gi, gd, gc, *_ = _run(ix, [g, g[::-1]], 6, 10, "min")
    assert gc.tolist() == [8, 8]
    assert gi[0, :8].tolist() == [4, 7, 2, 3, 5, 8, 1, 6]
    assert gd[0, :8].view(np.uint32).tolist() == [0xFF800000, 0xFF800000, 0x80000000, 0, 0x40E00000, 0x7F800000, 0x7FC00001, 0xFFC00002]
    assert gd[1, :8].view(np.uint32).tolist() == [0xFF800000, 0xFF800000, 0x80000000, 0x80000000, 0x40E00000, 0x7F800000, 0xFFC00002, 0x7FC00001]
    _check(ix, [g, g[::-1], [g[1], g[0], g[2]]], 6, (1, 3, 8, 12), "min", what="special")


def test_short_counts_and_counts_above_ld(ix):
    rng = np.random.default_rng(11)
    groups = [[rng.permutation(400)[:130].tolist() for _ in range(3)] for _ in range(2)]
    for mode in ("rrf", "min"):
        _check(ix, groups, 130, (1, 50, 400), mode, counts=[130, 40, 100000, 0, 1, 129], what="counts")


def test_id_offset(ix):
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(12)
    off = (1 << 33) + 5
    ix.set_id_offset(off)
    try:
        groups = [[rng.permutation(N)[:100].tolist() for _ in range(3)], [[N - 1, 0], [0, N - 1]]]
        for mode in ("rrf", "min"):
            exp = _check(ix, groups, 100, (1, 30, 300), mode, id_offset=off, what="offset")
            assert min(exp[0][0]) >= off
        with pytest.raises(vdb.VdbError, match="no row of this index"):  # local numbers are no rows of the index now
            _run(ix, groups, 100, 5, "rrf", id_offset=0)
    finally:
        ix.set_id_offset(0)


@pytest.mark.parametrize("S,in_lds", ((4, 1), (5, 0), (16, 0)))
def test_both_table_places(ix, S, in_lds):
    """4 lists x 1024 fill the largest table LDS holds; 5 x 1024 is the first on the scratch path; 16 x 1024 is the cap"""
    ld = 1024
    code, s_max, lg, lds, scratch, _ = _plan([0, S, S + 2], 1, ld)
    assert (code, s_max, lds) == (0, S, in_lds) and lg == {4: 13, 5: 14, 16: 15}[S] and scratch == (0 if in_lds else 16 << lg)
    rng = np.random.default_rng(S)
    g0 = [rng.permutation(N)[:ld].tolist() for _ in range(S)]
    g1 = [rng.permutation(N)[:ld].tolist() for _ in range(2)]  # a second slice of the scratch buffer
    w = rng.uniform(0.5, 2.0, size=S + 2).astype(np.float32)
    _check(ix, [g0, g1], ld, (1, 10, 1499, 1505), "rrf", weights=w, what=f"S={S}")
    dg = [[(l, rng.integers(0, 200, size=ld).astype(np.float32)) for l in g] for g in (g0, g1)]
    _check(ix, dg, ld, (10, 1500), "min", what=f"S={S}")
    if S == 16:  # all 16384 entries distinct is impossible on 1500 rows; the union is the whole table
        assert len(_expected(*_pack([g0, g1], ld)[:4], ld, 0, "rrf", None, 60.0)[0]) == N


def test_refusals_leave_outputs_and_counters_untouched(ix):
    import torch

    import lab_1806_vec_db_amd as vdb

    rows = list(range(40))
    before = {s: ix.get_stat(s) for s in STATS}

    def untouched():
        gi, gd, gc = _run.last
        return (gi == SENT).all() and (gd == -7.0).all() and (gc == SENT).all()

    def refused(match, *a, **kw):
        with pytest.raises(vdb.VdbError, match=match):
            _run(ix, *a, **kw)
        assert untouched(), match

    refused("no row of this index", [[rows, rows + [N]]], 64, 5, "rrf")       # inside the count
    refused("no row of this index", [[rows], [[N + 9]]], 64, 5, "min")
    _run(ix, [[rows + [N]]], 64, 5, "rrf", counts=[40])                        # beyond the count: not read
    assert _run.last[2][0] == 5
    refused("mode", [[rows]], 64, 5, 7)
    refused("start at 0", [[rows]], 64, 5, "rrf", lims=[1, 1])
    refused("not decrease", [[rows], [rows]], 64, 5, "rrf", lims=[0, 2, 1])
    refused("at least one sub-query", [[rows], [rows]], 64, 5, "rrf", lims=[0, 0, 2])
    refused("at most 32", [[rows] * 33], 64, 5, "rrf")
    _run(ix, [[rows] * 32], 64, 5, "rrf")
    refused("at most 4096", [[rows]], 4097, 5, "rrf")
    refused("at most 16384", [[rows] * 5], 4096, 5, "rrf")
    refused("at most 16384", [[rows] * 17], 1024, 5, "rrf")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("weight", [[rows, rows]], 64, 5, "rrf", weights=[1.0, bad])
    refused("VDB_FUSE_RRF only", [[rows]], 64, 5, "min", weights=[1.0])
    for bad in (-1.0, float("nan"), float("inf")):
        refused("rrf_c", [[rows]], 64, 5, "rrf", c=bad)
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = t.data_ptr()
    with pytest.raises(vdb.VdbError, match="null"):
        ix.fuse_lists_device(0, p, p, [0, 1], 4, 2, p, p, p)
    u8 = vdb.GpuIndex(4, "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.zeros((8, 4), dtype=np.uint8))
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            u8.fuse_lists_device(p, p, p, [0, 1], 4, 2, p, p, p)
    finally:
        u8.close()
    assert not t.cpu().numpy().any()
    # nq == 0, k == 0 and empty lists: empty results
    ix.fuse_lists_device(0, 0, 0, [0], 4, 2, 0, 0, 0)
    gi, gd, gc, *_ = _run(ix, [[rows]], 64, 0, "rrf")
    assert gc[0] == 0 and (gi == SENT).all()
    gi, gd, gc, *_ = _run(ix, [[[], []], [[]]], 64, 3, "min")
    assert gc.tolist() == [0, 0] and not gi.any() and not gd.view(np.uint32).any()
    assert {s: ix.get_stat(s) for s in STATS} == before  # the list form counts nothing, refused or not


def test_two_threads(ix):
    rng = np.random.default_rng(21)
    jobs = []
    for t in range(2):
        groups = [[rng.permutation(600)[:257].tolist() for _ in range(3 + t)] for _ in range(20)]
        jobs.append((groups, "rrf" if t == 0 else "min"))
    out, err = [None, None], []

    def work(t):
        try:
            for _ in range(5):
                out[t] = _run_private(ix, *jobs[t])
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for t in range(2):
        gi, gd, gc, ids, dd, cnt, lm = out[t]
        for q in range(20):
            _compare((gi, gd, gc), _expected(ids, dd, cnt, lm, 257, q, jobs[t][1], None, 60.0), 50, q, f"thread {t}")


def _run_private(ix, groups, mode):
    """_run without the shared `last` slot, for the threads"""
    import torch

    ids, dd, cnt, lm = _pack(groups, 257)
    nq = len(lm) - 1
    t_ids, t_d, t_c = torch.from_numpy(ids.view(np.int64)).cuda(), torch.from_numpy(dd).cuda(), torch.from_numpy(cnt.view(np.int64)).cuda()
    o_i = torch.full((nq, 50), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, 50), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.fuse_lists_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), lm, 257, 50, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode=mode)
    torch.cuda.synchronize()
    return o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64), ids, dd, cnt, lm
