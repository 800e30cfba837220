"""GPU: k_like_build alone (GpuIndex.like_queries / like_queries_device, vdb_like_queries*) against tests/like_ref.py, the loop in
np.float32 scalars that restates the contract (tests/test_like_ref_cpu.py verifies it without a GPU).  Every element is compared bit
for bit; a NaN matches any NaN (IEEE 754 leaves the sign and payload of a produced NaN open: like_ref.same_floats)."""
import ctypes as C

import numpy as np
import pytest

import like_ref as R

pytestmark = pytest.mark.gpu

N = 300
# rows with a fixed role
NAN_ROW, PINF_ROW, NINF_ROW, NZERO_ROW, DENORM_ROW, BIG_ROW = 40, 41, 42, 43, 44, 45
SPECIAL = (NAN_ROW, PINF_ROW, NINF_ROW, NZERO_ROW, DENORM_ROW, BIG_ROW)
PLAIN = np.array([r for r in range(N) if r not in SPECIAL])
STATS = ("flat_like_calls", "flat_like_queries", "like_example_rows", "fetch_calls", "fetch_rows")
# (|P|, |N|) per dim: every length around the wave size where the reference loop stays cheap, fewer at the long rows
SMALL = [(p, g) for p in (1, 2, 3, 63, 64, 65) for g in (0, 1, 64)]
COMBOS = {1: SMALL + [(1024, 0), (960, 64)], 4: SMALL + [(1024, 0), (960, 64)], 5: SMALL + [(1024, 0)], 20: SMALL,
          960: [(1, 0), (2, 1), (3, 64), (63, 0), (64, 1), (65, 64)], 2049: [(1, 0), (2, 1), (3, 0), (65, 64)]}
SHAPES = [(dim, dist) for dim in (1, 4, 5, 20, 960, 2049) for dist in ("l2sqr", "cosine")]


def _base(dim):
    rng = np.random.default_rng(4100 + dim)
    base = rng.standard_normal((N, dim)).astype(np.float32)
    base[NAN_ROW, dim // 2] = np.nan
    base[PINF_ROW, 0] = np.inf
    base[NINF_ROW, dim - 1] = -np.inf
    base[NZERO_ROW] = -0.0
    base[DENORM_ROW] = np.float32(1e-42) * (1 + np.arange(dim) % 7)
    base[BIG_ROW] = np.float32(2.5e38)
    return base


class Env:
    def __init__(self, dim, dist):
        import lab_1806_vec_db_amd as vdb

        self.dim, self.base = dim, _base(dim)
        self.ix = vdb.GpuIndex(dim, dist, device=0)
        self.ix.batch_add(self.base)
        rng = np.random.default_rng(7 * dim + len(dist))
        self.pos, self.neg = [], []
        for p, g in COMBOS[dim]:
            self.pos.append(rng.choice(PLAIN, size=p).tolist())  # (with replacement: repeats occur by themselves in the long lists)
            self.neg.append(rng.choice(PLAIN, size=g).tolist())
        # the same id repeated, the first and the last row of the table, the special rows on both sides
        extra = [([7, 7, 7], []), ([7, 9, 7], [9, 9]), ([0], []), ([N - 1], []), ([0, N - 1], [N - 1, 0]), ([NZERO_ROW], []), ([NZERO_ROW, NZERO_ROW], [NZERO_ROW]),
                 ([DENORM_ROW], []), ([DENORM_ROW, DENORM_ROW, DENORM_ROW], [DENORM_ROW]), ([NAN_ROW, 3], []), ([3], [NAN_ROW]), ([PINF_ROW, NINF_ROW], []),
                 ([PINF_ROW, 5], [PINF_ROW]), ([NINF_ROW], [6]), ([BIG_ROW, BIG_ROW], []), ([BIG_ROW], [3]), ([3], [BIG_ROW, BIG_ROW])]
        for p, g in extra:
            self.pos.append(p)
            self.neg.append(g)
        self.ref = R.like_queries(self.base, self.pos, self.neg)  # computed once, shared, never changed


_envs = {}


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def env(request):
    if request.param not in _envs:
        _envs[request.param] = Env(*request.param)
    return _envs[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for e in _envs.values():
        e.ix.close()
    _envs.clear()


def _stats(ix):
    return {s: ix.get_stat(s) for s in STATS}


def _lims(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)


def _device_queries(ix, pos, neg, id_offset=0, pad=1, with_neg=True):
    """the device form into a buffer whose payload starts `pad` floats in (4-byte aligned, not 16) with sentinels around it
    -> (queries, the floats in front, the floats behind)"""
    import torch

    nq, dim = len(pos), ix.dim
    flat = lambda ls: torch.from_numpy((np.asarray([r for x in ls for r in x], dtype=np.uint64) + np.uint64(id_offset)).view(np.int64)).cuda()
    t_p, t_n = flat(pos), flat(neg)
    buf = torch.full((nq * dim + pad + 5,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.like_queries_device(_lims(pos), t_p.data_ptr() if t_p.numel() else 0, _lims(neg) if with_neg else None, t_n.data_ptr() if t_n.numel() else 0, nq,
                               buf.data_ptr() + 4 * pad)
    finally:
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        _device_queries.last = h
    return h[pad:pad + nq * dim].reshape(nq, dim), h[:pad], h[pad + nq * dim:]


def test_host_form_matches_reference(env):
    s0 = _stats(env.ix)
    got = env.ix.like_queries(env.pos, env.neg)
    assert got.shape == env.ref.shape
    for q in range(len(env.pos)):
        assert R.same_floats(got[q], env.ref[q]), (q, len(env.pos[q]), len(env.neg[q]))
    s1 = _stats(env.ix)
    assert s1["like_example_rows"] - s0["like_example_rows"] == sum(map(len, env.pos)) + sum(map(len, env.neg))
    assert s1["flat_like_calls"] == s0["flat_like_calls"] and s1["flat_like_queries"] == s0["flat_like_queries"]
    # one positive, no negatives: the row itself, -0.0 made +0.0
    q = env.pos.index([NZERO_ROW])
    assert not np.signbit(got[q]).any() and not got[q].any()
    q = env.pos.index([0])
    assert got[q].tobytes() == env.base[0].tobytes()


def test_device_form_with_id_offset_and_unaligned_output(env):
    env.ix.set_id_offset(1000)
    try:
        got, front, back = _device_queries(env.ix, env.pos, env.neg, id_offset=1000, pad=1)
    finally:
        env.ix.set_id_offset(0)
    assert (front == -7.0).all() and (back == -7.0).all()
    for q in range(len(env.pos)):
        assert R.same_floats(got[q], env.ref[q]), (q, len(env.pos[q]), len(env.neg[q]))


def test_no_negatives_at_all_and_ragged_batches(env):
    """neg_lims == NULL, and nq = 1, 2 and 257 with ragged list lengths"""
    rng = np.random.default_rng(env.dim)
    lens = 1 + (np.arange(257) * 5) % (4 if env.dim > 20 else 9)
    pos = [rng.choice(PLAIN, size=int(n)).tolist() for n in lens]
    neg = [rng.choice(PLAIN, size=int(n) % 3).tolist() for n in lens]
    if env.dim > 20:  # (the reference loop: fewer of the long rows)
        pos, neg = pos[:40], neg[:40]
    ref_pn = R.like_queries(env.base, pos, neg)
    ref_p = R.like_queries(env.base, pos)
    for nq in (1, 2, len(pos)):
        got = env.ix.like_queries(pos[:nq], neg[:nq])
        assert R.same_floats(got, ref_pn[:nq]), nq
        got = env.ix.like_queries(pos[:nq])
        assert R.same_floats(got, ref_p[:nq]), nq
        got, front, back = _device_queries(env.ix, pos[:nq], [[] for _ in range(nq)], pad=3, with_neg=False)
        assert R.same_floats(got, ref_p[:nq]) and (front == -7.0).all() and (back == -7.0).all(), nq
    assert env.ix.like_queries([]).shape == (0, env.dim)


def test_fold_order_is_the_list_order():
    import lab_1806_vec_db_amd as vdb

    rows = np.array([[1e8], [1.0], [-1e8]], dtype=np.float32)
    ix = vdb.GpuIndex(1, "l2sqr", device=0)
    try:
        ix.batch_add(rows)
        got = ix.like_queries([[0, 1, 2], [0, 2, 1]])
        assert got.view(np.uint32).ravel().tolist() == [0, np.float32(np.float32(1.0) / np.float32(3.0)).view(np.uint32)]
        assert R.same_floats(got, R.like_queries(rows, [[0, 1, 2], [0, 2, 1]]))
        got, _, _ = _device_queries(ix, [[0, 1, 2], [0, 2, 1]], [[], []])
        assert got.view(np.uint32).ravel().tolist() == [0, 0x3EAAAAAB]
    finally:
        ix.close()


def test_output_is_a_query_for_the_device_searches(env):
    import torch

    pos, neg = [[3, 5, 8], [10], [11, 12]], [[20], [], [21, 22, 23]]
    nq, k = 3, 7
    host_q = env.ix.like_queries(pos, neg)
    ei, ed, ec = env.ix.flat_knn(host_q, k)
    flat = lambda ls: torch.from_numpy(np.asarray([r for x in ls for r in x], dtype=np.int64)).cuda()
    t_p, t_n = flat(pos), flat(neg)
    d_q = torch.zeros((nq, env.dim), dtype=torch.float32, device="cuda")
    o_i = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    o_d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    o_c = torch.zeros((nq,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    env.ix.like_queries_device(_lims(pos), t_p.data_ptr(), _lims(neg), t_n.data_ptr(), nq, d_q.data_ptr())
    env.ix.flat_knn_device(d_q.data_ptr(), nq, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())
    torch.cuda.synchronize()
    assert d_q.cpu().numpy().tobytes() == host_q.tobytes()
    assert np.array_equal(o_c.cpu().numpy().view(np.uint64), ec)
    assert np.array_equal(o_i.cpu().numpy().view(np.uint64), ei) and o_d.cpu().numpy().tobytes() == np.ascontiguousarray(ed).tobytes()


def _raw(ix, pl, pr, nl, nr, nq, out):
    from lab_1806_vec_db_amd import _lib as L

    a = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.uint64)
    pl, pr, nl, nr = a(pl), a(pr), a(nl), a(nr)
    p = lambda x: None if x is None else x.ctypes.data_as(L.u64p)
    return ix._lib.vdb_like_queries(ix._h, p(pl), p(pr), p(nl), p(nr), nq, out.ctypes.data_as(L.f32p))


def test_every_refusal_leaves_outputs_and_counters_alone():
    import torch

    import lab_1806_vec_db_amd as vdb

    dim = 8
    base = np.random.default_rng(3).standard_normal((50, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr", device=0)
    u8 = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    try:
        ix.batch_add(base)
        u8.batch_add_u8((np.abs(base) * 50).astype(np.uint8))
        s0, s0_u8 = _stats(ix), _stats(u8)
        out = np.full((2, dim), -7.0, dtype=np.float32)
        many = list(range(50)) * 21  # 1050 entries
        bad = [
            ([1, 2, 3], [1, 2, 3], None, None),              # limits that do not start at 0
            ([0, 2, 1], [1, 2, 3], None, None),              # a descent
            ([0, 0, 2], [1, 2], None, None),                 # a query without a positive
            ([0, 1, 1026], many[:1026], None, None),         # 1025 examples
            ([0, 1, 2], [1, 2], [0, 1000, 2024], many[:1012] * 2),  # 1 + 1024 with the negatives
            ([0, 1, 2], None, None, None),                   # a NULL list with entries
            ([0, 1, 2], [1, 2], [0, 1, 1], None),
            ([0, 1, 2], [1, 2], [5, 5, 5], [1] * 5),         # the negatives' limits are checked as the positives'
            ([0, 1, 2], [1, 50], None, None),                # a row that is no row of the index
            ([0, 1, 2], [1, 2], [0, 0, 1], [1 << 40]),
        ]
        for pl, pr, nl, nr in bad:
            assert _raw(ix, pl, pr, nl, nr, 2, out) != 0, (pl, nl)
            assert (out == -7.0).all()
        assert _raw(ix, None, None, None, None, 2, out) != 0
        assert _raw(u8, [0, 1, 2], [1, 2], None, None, 2, out) != 0 and (out == -7.0).all()
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            u8.like_queries([[1]])
        with pytest.raises(vdb.VdbError, match="at least one positive"):
            ix.like_queries([[1], []])
        with pytest.raises(vdb.VdbError, match="no row of this index"):
            ix.like_queries([[1], [50]])
        # the device form: a bad id on either side is found on the device, nothing is gathered, the output stays
        ix.set_id_offset(100)
        try:
            for pos, neg in (([[101], [150]], [[], []]), ([[101], [99]], [[], []]), ([[101], [102]], [[103], [1 << 50]])):
                with pytest.raises(vdb.VdbError, match="no row of this index"):
                    _device_queries(ix, pos, neg)
                assert (_device_queries.last == -7.0).all()
            t = torch.zeros(4, dtype=torch.int64, device="cuda")
            with pytest.raises(vdb.VdbError, match="8-byte aligned"):
                ix.like_queries_device([0, 1], t.data_ptr() + 4, None, 0, 1, t.data_ptr())
            with pytest.raises(vdb.VdbError, match="null positives"):
                ix.like_queries_device([0, 1], 0, None, 0, 1, t.data_ptr())
        finally:
            ix.set_id_offset(0)
        assert _stats(ix) == s0 and _stats(u8) == s0_u8
        assert _raw(ix, [0], None, None, None, 0, out) == 0 and (out == -7.0).all()  # nq == 0: nothing to do
    finally:
        ix.close()
        u8.close()
