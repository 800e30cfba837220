"""GPU: k_vote_lists alone (GpuIndex.vote_lists_device, vdb_vote_lists_device) over hand-made hit lists on a 300 x 8 index, every output
compared bit for bit with vote_ref below -- a numpy f32 loop that applies the rule of the vote to one list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 300
NONE = 0xFFFFFFFF
C_MIX, C_ONE, C_64, C_130, C_EDGE, C_NEVER, C_COLLIDE, C_FREE = 0, 1, 2, 3, 4, 5, 6, 7
F = np.float32


def order_key(x):  # the order-preserving integer image of an f32 (no NaN score can arise)
    u = int(np.array(x + F(0.0), dtype=F).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def vote_ref(codes, dists, c, mode, eps):
    """codes / dists of one list in list order -> (code [c], score [c], votes [c], values written, voters)"""
    tally, voters = {}, 0  # code -> [score, votes, first]
    with np.errstate(all="ignore"):
        for pos, (v, d) in enumerate(zip(codes, dists)):
            if int(v) == NONE:
                continue
            voters += 1
            w = F(1.0) if mode == "uniform" else (F(0.0) if np.isnan(d) else F(1.0) / F(F(d) + F(eps)))
            s = tally.setdefault(int(v), [F(0.0), 0, pos])
            s[0], s[1] = F(s[0] + w), s[1] + 1
    ranked = sorted(tally.items(), key=lambda it: (-order_key(it[1][0]), it[1][2]))[:c]
    code, score, votes = np.full(c, NONE, np.uint32), np.zeros(c, F), np.zeros(c, np.uint32)
    for i, (v, s) in enumerate(ranked):
        code[i], score[i], votes[i] = v, s[0], s[1]
    return code, score, votes, len(ranked), voters


def _hash(code, lg):  # vote_plan.hpp: vote_hash
    return ((code * 2654435761) & 0xFFFFFFFF) >> (32 - lg)


@pytest.fixture(scope="module")
def env():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(5)
    ix = vdb.GpuIndex(8, "l2sqr", device=0)
    ix.batch_add(rng.random((N, 8), dtype=F))
    r = np.arange(N)
    collide = [c for c in range(1, 1 << 20) if _hash(c, 13) == _hash(1, 13)][:6]  # one probe path at every table size (a prefix of the hash)
    assert len(collide) == 6
    cols = {
        C_MIX: rng.choice(np.array([3, 4, 5, 6, 9, NONE], dtype=np.uint32), size=N, p=[0.4, 0.2, 0.1, 0.1, 0.05, 0.15]),
        C_ONE: np.full(N, 7, np.uint32),
        C_64: (r % 64).astype(np.uint32),
        C_130: (r % 130 + 1000).astype(np.uint32),
        C_EDGE: np.where(r % 3 == 0, 0, np.where(r % 3 == 1, 0xFFFFFFFE, NONE)).astype(np.uint32),
        C_COLLIDE: np.array(collide, dtype=np.uint32)[r % 6],
    }
    for c, v in cols.items():
        ix.set_labels(c, v)
    cols[C_NEVER] = np.full(N, NONE, np.uint32)
    yield ix, cols, rng
    ix.close()


def _run(ix, rows, dists, ld, column, c, mode, eps=1e-6, id_offset=0, out_ptr=True):
    """rows / dists: per query a list in LOCAL rows -> the five outputs, pre-filled with a sentinel; _run.last keeps them on a raise"""
    import torch

    nq = len(rows)
    ids = np.full((nq, ld), 0xDEAD0000, dtype=np.uint64)  # (beyond a count: never read)
    dd = np.zeros((nq, ld), dtype=F)
    cnt = np.array([len(x) for x in rows], dtype=np.uint64)
    for q in range(nq):
        ids[q, :len(rows[q])] = np.asarray(rows[q], dtype=np.int64) + id_offset
        dd[q, :len(rows[q])] = dists[q]
    cc = max(c, 1)
    t_in = [torch.from_numpy(a).cuda() for a in (ids.view(np.int64), dd, cnt.view(np.int64))]
    outs = [torch.full((nq, cc), -7, dtype=torch.int32, device="cuda"), torch.full((nq, cc), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((nq, cc), -7, dtype=torch.int32, device="cuda"), torch.full((nq,), -7, dtype=torch.int64, device="cuda"),
            torch.full((nq,), -7, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    try:
        ix.vote_lists_device(*[t.data_ptr() for t in t_in], nq, ld, column, c, outs[0].data_ptr(), outs[1].data_ptr() if out_ptr else 0,
                             *[t.data_ptr() for t in outs[2:]], mode=mode, eps=eps)
    finally:
        torch.cuda.synchronize()
        h = [t.cpu().numpy() for t in outs]
        _run.last = (h[0].view(np.uint32), h[1], h[2].view(np.uint32), h[3].view(np.uint64), h[4].view(np.uint64))
    return _run.last


def _check(ix, col, rows, dists, ld, column, c, mode, eps=1e-6, id_offset=0):
    got = _run(ix, rows, dists, ld, column, c, mode, eps, id_offset)
    for q in range(len(rows)):
        code, score, votes, n, voters = vote_ref(col[np.asarray(rows[q], dtype=np.int64)], dists[q], c, mode, eps)
        assert got[0][q].tolist() == code.tolist(), (q, got[0][q], code)
        assert got[1][q].view(np.uint32).tolist() == score.view(np.uint32).tolist(), (q, got[1][q], score)
        assert got[2][q].tolist() == votes.tolist()
        assert (int(got[3][q]), int(got[4][q])) == (n, voters)
    return got


def _list(rng, length):
    """a list of `length` rows (repeats allowed: the kernel walks what it is given) with ascending distances, some of them equal"""
    d = np.sort(rng.random(length, dtype=F))
    d[1::7] = d[0::7][:len(d[1::7])]
    return rng.integers(0, N, size=length), d


@pytest.mark.parametrize("mode", ["uniform", "inverse"])
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 130, 4096])
def test_lengths_and_c(env, length, mode):
    ix, cols, rng = env
    ld = max(length, 1)
    rows, d = _list(rng, length)
    before = ix.get_stat("flat_vote_queries"), ix.get_stat("flat_vote_scratch")
    for c in sorted({1, min(3, ld), ld}):
        _check(ix, cols[C_MIX], [rows, rows[::-1]], [d, d], ld, C_MIX, c, mode)
    calls = len({1, min(3, ld), ld})
    assert ix.get_stat("flat_vote_queries") - before[0] == 2 * calls
    assert ix.get_stat("flat_vote_scratch") - before[1] == (2 * calls if length == 4096 else 0)  # 2^13 slots: the table left LDS


@pytest.mark.parametrize("mode", ["uniform", "inverse"])
@pytest.mark.parametrize("column", [C_ONE, C_64, C_130, C_EDGE, C_NEVER, C_COLLIDE])
def test_label_shapes(env, column, mode):
    ix, cols, rng = env
    rows, d = _list(rng, 200)
    seq = np.arange(200)  # rows in order: 64 distinct values in every tile of C_64, 130 distinct values in C_130
    for c in (1, 200):
        got = _check(ix, cols[column], [rows, seq], [d, d], 200, column, c, mode)
    if column == C_NEVER:
        assert got[3].tolist() == [0, 0] and got[4].tolist() == [0, 0]
    # a list of 4096 over the same column: the scratch table, 64 tiles
    rows, d = _list(rng, 4096)
    _check(ix, cols[column], [rows], [d], 4096, column, 5, mode)


def _relabel(ix, codes_by_row):
    col = np.full(N, NONE, np.uint32)
    for r, c in codes_by_row.items():
        col[r] = c
    ix.set_labels(C_FREE, col)
    return col


def test_fold_across_tiles_and_order(env):
    ix, _, _ = env
    # value 1 votes at lane 63 and at lane 0 of the next tile only; value 2 everywhere else
    col = _relabel(ix, {r: (1 if r in (63, 64) else 2) for r in range(130)})
    d = (np.arange(130) * 0.01).astype(F)
    for mode in ("uniform", "inverse"):
        got = _check(ix, col, [np.arange(130)], [d], 130, C_FREE, 2, mode)
        assert got[0][0].tolist() == [2, 1] and got[2][0].tolist() == [128, 2]
    # INVERSE, eps = 2^-30: value 1 has the weights 2^24, 1, 1, 1 at positions 0, 10, 70, 130 -- 2^24 swallows every 1 in list order,
    # while any order that adds the ones first ends at 2^24 + 4
    eps = 2.0 ** -30
    at = [0, 10, 70, 130]
    col = _relabel(ix, {r: (1 if r in at else 2) for r in range(140)})
    d = np.full(140, 3.0, dtype=F)
    d[at] = [2.0 ** -24 - 2.0 ** -30, 1.0, 1.0, 1.0]
    w = [F(1.0) / F(F(x) + F(eps)) for x in d[at]]
    fwd = F(F(F(F(0.0) + w[0]) + w[1]) + w[2]) + w[3]
    rev = F(F(F(F(0.0) + w[3]) + w[2]) + w[1]) + w[0]
    assert F(fwd) != F(rev) and vote_ref(col[:140], d, 2, "inverse", eps)[1][0] == F(fwd)
    got = _check(ix, col, [np.arange(140)], [d], 140, C_FREE, 2, "inverse", eps)
    assert got[0][0][0] == 1 and got[1][0][0] == F(fwd)


def test_tie_first_and_special_distances(env):
    ix, _, _ = env
    # values 8 and 9 with two votes each: 9's first voter is nearer
    col = _relabel(ix, {0: 9, 1: 8, 2: 8, 3: 9, 4: 5})
    got = _check(ix, col, [np.arange(5)], [np.arange(5, dtype=F)], 5, C_FREE, 3, "uniform")
    assert got[0][0].tolist() == [9, 8, 5]
    # NaN weighs 0 and still counts, +inf gives 0, 0.0 gives 1 / eps
    col = _relabel(ix, {0: 1, 1: 1, 2: 2, 3: 2, 4: 3, 5: 3})
    d = np.array([0.0, np.nan, np.inf, 1.0, np.nan, np.nan], dtype=F)
    got = _check(ix, col, [np.arange(6)], [d], 6, C_FREE, 3, "inverse")
    assert got[0][0].tolist() == [1, 2, 3] and got[2][0].tolist() == [2, 2, 2] and got[1][0][2] == 0.0


def test_id_offset_and_repeat(env):
    import lab_1806_vec_db_amd as vdb

    _, cols, rng = env
    ix = vdb.GpuIndex(8, "l2sqr", device=0)
    try:
        ix.batch_add(rng.random((N, 8), dtype=F))
        ix.set_id_offset(1000)
        ix.set_labels(C_MIX, cols[C_MIX])
        rows, d = _list(rng, 130)
        a = _check(ix, cols[C_MIX], [rows], [d], 130, C_MIX, 3, "inverse", id_offset=1000)
        b = _run(ix, [rows], [d], 130, C_MIX, 3, "inverse", id_offset=1000)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))  # the same bits on a second call
        with pytest.raises(vdb.VdbError, match="no row of this index"):
            _run(ix, [rows], [d], 130, C_MIX, 3, "inverse", id_offset=0)  # ids below the offset
    finally:
        ix.close()


@pytest.mark.parametrize("bad", ["id", "ld0", "ld_long", "c0", "c_over", "mode", "eps0", "eps_inf", "eps_nan", "column", "null"])
def test_refusals(env, bad):
    import lab_1806_vec_db_amd as vdb

    ix, _, rng = env
    rows, d = _list(rng, 70)
    kw = dict(rows=[rows], dists=[d], ld=70, column=C_MIX, c=2, mode="uniform", eps=1e-6)
    if bad == "id":
        kw["rows"] = [np.concatenate([rows[:69], [N]])]
    kw.update({"ld0": dict(ld=0, rows=[rows[:0]], dists=[d[:0]]), "ld_long": dict(ld=4097), "c0": dict(c=0), "c_over": dict(c=71), "mode": dict(mode=7),
               "eps0": dict(mode="inverse", eps=0.0), "eps_inf": dict(mode="inverse", eps=float("inf")),
               "eps_nan": dict(mode="inverse", eps=float("nan")), "column": dict(column=16), "null": dict(out_ptr=False)}.get(bad, {}))
    if kw["ld"] == 0:  # (torch has no tensor of zero columns to point at: one column, the library is told ld = 0)
        import torch

        z = torch.zeros(4, dtype=torch.int64, device="cuda")
        before = ix.get_stat("flat_vote_queries")
        with pytest.raises(vdb.VdbError):
            ix.vote_lists_device(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 0, C_MIX, 1, *[z.data_ptr()] * 5)
        assert ix.get_stat("flat_vote_queries") == before and not z.cpu().any()
        return
    before = ix.get_stat("flat_vote_queries"), ix.get_stat("flat_vote_scratch")
    with pytest.raises(vdb.VdbError):
        _run(ix, **kw)
    assert (ix.get_stat("flat_vote_queries"), ix.get_stat("flat_vote_scratch")) == before
    got = _run.last
    assert (got[0] == 0xFFFFFFF9).all() and (got[1] == -7.0).all() and (got[2] == 0xFFFFFFF9).all()
    assert (got[3].view(np.int64) == -7).all() and (got[4].view(np.int64) == -7).all()
