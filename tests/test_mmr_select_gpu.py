"""GPU: k_mmr_select alone (GpuIndex.mmr_select_device, vdb_mmr_select_device) over hand-made candidate lists against tests/mmr_ref.py,
the reference walk in np.float32 over the CPU oracle's pair distances (tests/test_mmr_ref_cpu.py verifies it without a GPU).  The lists
are walked as given -- any order of ids, any distances, position is the tie order -- and every comparison is bit for bit: ids, selection
order, distances as f32 bit patterns (the kernel only moves them), counts, zeros behind the count."""
import numpy as np
import pytest

import mmr_ref as R

pytestmark = pytest.mark.gpu

N = 320
LAMBDAS = (0.0, 0.25, 0.5, 0.75, 1.0)
SHAPES = [(dim, dist, kind) for dim in (4, 5, 20, 960) for dist, kind in (("l2sqr", 0), ("cosine", 1))]  # (5: no multiple of 4 -- the scalar path)
SENT = np.uint64(-7 & 0xFFFFFFFFFFFFFFFF)
# rows with a fixed role
ZERO, NAN_ROW, PINF_ROW, NINF_ROW = 50, 60, 61, 62
TWINS_A, TWINS_B = (100, 101, 102, 103), (110, 111, 112)  # two groups of identical rows, far from the random ones
PLAIN = np.array([r for r in range(N) if r not in (ZERO, NAN_ROW, PINF_ROW, NINF_ROW) + TWINS_A + TWINS_B])


def _base(dim):
    rng = np.random.default_rng(900 + dim)
    base = rng.standard_normal((N, dim)).astype(np.float32)
    base[ZERO] = 0.0
    base[NAN_ROW, dim // 2] = np.nan
    base[PINF_ROW, 0] = np.inf
    base[NINF_ROW, dim - 1] = -np.inf
    base[list(TWINS_A)] = base[TWINS_A[0]] * np.float32(9.0)
    base[list(TWINS_B)] = -base[TWINS_B[0]] * np.float32(7.0)
    return base


class Env:
    def __init__(self, dim, dist, kind, base=None):
        import lab_1806_vec_db_amd as vdb

        self.base = _base(dim) if base is None else base
        self.ix = vdb.GpuIndex(dim, dist, device=0)
        self.ix.batch_add(self.base)
        self.rd = R.RowDist(self.base, kind)
        self.rng = np.random.default_rng(17 * dim + kind)
        self._walks = {}

    def selection(self, rows, d, lam, k):
        """the reference's selection of min(k, len(rows)) positions; the longest one computed so far per (list, lambda) is kept, because
        a smaller k is its prefix (greedy: no step depends on k; tests/test_mmr_ref_cpu.py::test_smaller_k_is_a_prefix)"""
        key = (tuple(int(r) for r in rows), np.asarray(d, dtype=np.float32).tobytes(), float(lam))
        kk = min(k, len(rows))
        if key not in self._walks or len(self._walks[key]) < kk:
            self._walks[key] = R.walk_rows(self.rd, rows, d, kk, lam)
        return self._walks[key][:kk]


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


def _run(ix, lists, dists, ld, k, lam, id_offset=0, counts=None):
    """lists: per query LOCAL rows, dists: per query f32 distances; -> (idx, dist, cnt) from the device, outputs pre-filled with a sentinel"""
    import torch

    nq = len(lists)
    ids = np.full((nq, max(ld, 1)), 0xDEAD, dtype=np.uint64)  # (beyond a count: never read -- 0xDEAD + offset is no row at all)
    dd = np.full((nq, max(ld, 1)), -3.0, dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q, rows in enumerate(lists):
        ids[q, :len(rows)] = np.asarray(rows, dtype=np.uint64) + np.uint64(id_offset)
        dd[q, :len(rows)] = dists[q]
        cnt[q] = len(rows)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.uint64)
    kk = max(k, 1)
    t_ids = torch.from_numpy(ids.view(np.int64)).cuda()
    t_d = torch.from_numpy(dd).cuda()
    t_c = torch.from_numpy(cnt.view(np.int64)).cuda()
    o_i = torch.full((nq, kk), -7, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, kk), -7.0, dtype=torch.float32, device="cuda")
    o_c = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.mmr_select_device(t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), nq, ld, k, lam, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())
    finally:
        torch.cuda.synchronize()
        _run.last = (o_i.cpu().numpy().view(np.uint64), o_d.cpu().numpy(), o_c.cpu().numpy().view(np.uint64))
    return _run.last


def _check(env, lists, dists, ld, k, lam, id_offset=0, what=""):
    gi, gd, gc = _run(env.ix, lists, dists, ld, k, lam, id_offset)
    kk = max(k, 1)
    for q, rows in enumerate(lists):
        rows = np.asarray(rows, dtype=np.int64)
        d = np.asarray(dists[q], dtype=np.float32)
        sel = env.selection(rows, d, lam, k)
        ei = np.zeros(kk, dtype=np.uint64)
        ed = np.zeros(kk, dtype=np.float32)
        ei[:len(sel)] = rows[sel].astype(np.uint64) + np.uint64(id_offset)
        ed[:len(sel)] = d[sel]
        assert int(gc[q]) == len(sel), (what, q, gc[q], len(sel))
        assert gi[q].tolist() == ei.tolist(), (what, q, lam, k, gi[q][:8], ei[:8])
        assert np.array_equal(gd[q].view(np.uint32), ed.view(np.uint32)), (what, q)
    return gi, gd, gc


def _dists(env, n):
    return (env.rng.random(n) * 4.0).astype(np.float32)  # in no order: the list is walked as given


LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 200)


def test_lengths_k_and_lambda(env):
    """every list length around the wave and the workgroup size in ONE call (the counts differ within it, most are shorter than ld),
    k = 1, 2, ld - 1, ld, every lambda; the lists are in no order"""
    lists = [env.rng.choice(PLAIN, size=n, replace=False) for n in LENGTHS]
    dists = [_dists(env, n) for n in LENGTHS]
    for lam in LAMBDAS:
        for k in (200, 199, 2, 1):
            _, _, gc = _check(env, lists, dists, 200, k, lam, what=("lengths", lam, k))
            assert gc.tolist() == [min(k, n) for n in LENGTHS]
    # lists of up to 64 positions: the one-wave launch
    for lam in (0.0, 0.5):
        _check(env, lists[:5], dists[:5], 64, 64, lam, what=("one wave", lam))
        _check(env, lists[:4], dists[:4], 63, 62, lam, what=("one wave 63", lam))
    _check(env, lists[:2], dists[:2], 1, 1, 0.5, what="ld 1")
    _check(env, lists[:3], dists[:3], 2, 2, 0.5, what="ld 2")
    gi, gd, gc = _run(env.ix, lists[:3], dists[:3], 2, 0, 0.5)  # k = 0: nothing is written but the counts
    assert (gc == 0).all() and (gi == SENT).all() and (gd == -7.0).all()


@pytest.mark.parametrize("lo,hi,n", [(63, 64, 130), (62, 63, 130), (64, 65, 130), (127, 128, 200), (255, 256, 300), (0, 299, 300)])
def test_tie_partners_across_lanes_and_waves(env, lo, hi, n):
    """two identical rows with equal list distances, far from position 0 and nearer the query than everything else: their scores are equal
    bit for bit at step 1 (D = the same, d = the same), so position decides -- with the partners at lane 63 and lane 0 of the next wave,
    at the last thread and the first thread's second position, and at both ends of the list"""
    rows = env.rng.choice(PLAIN, size=n, replace=False)
    d = (1.0 + env.rng.random(n)).astype(np.float32)
    d[0] = 0.5
    for twins in (TWINS_A, TWINS_B):
        if lo == 0:  # position 0 is selected first whatever it is: the partners are 1 and the end
            rows[1], rows[hi] = twins[0], twins[1]
            d[1] = d[hi] = 0.75
        else:
            rows[lo], rows[hi] = twins[0], twins[1]
            d[lo] = d[hi] = 0.75
        first = lo if lo else 1
        for lam in (0.25, 0.5, 1.0):
            gi, _, _ = _check(env, [rows, rows[::-1].copy()], [d, d[::-1].copy()], n, 4, lam, what=("twins", lo, hi, lam))
            if lam == 1.0:
                assert gi[0, 1] == rows[first] and gi[0, 2] == rows[hi]  # equal distances: the lower position, then its partner


def test_identical_rows_same_id_twice_and_equal_distances(env):
    grp = list(TWINS_A) + list(TWINS_B)
    lists = [np.array(grp * 10)[:66],                                  # every row a copy of one of two vectors, ids repeat
             np.concatenate([PLAIN[:40], PLAIN[:40]]),                 # the same id twice: D = 0 against itself
             np.array([PLAIN[3]] * 65),                                # one row only
             env.rng.choice(PLAIN, size=129, replace=False)]
    dists = [_dists(env, 66), _dists(env, 80), np.full(65, 2.5, dtype=np.float32), np.full(129, 1.0, dtype=np.float32)]  # (the last two: all equal)
    for lam in LAMBDAS:
        for k in (129, 66, 3):
            _check(env, lists, dists, 129, k, lam, what=("identical", lam, k))
    gi, _, gc = _check(env, lists[2:3], dists[2:3], 65, 65, 0.5)
    assert gc[0] == 65 and (gi[0] == PLAIN[3]).all()


def test_zero_nan_and_inf_rows(env):
    """a zero row (Cosine: the clamped denominator), rows with a NaN and with +-inf components at the list's start and end: pair
    distances that are NaN (ignored by the min) or inf, scores that are NaN (counted as +inf)"""
    mid = env.rng.choice(PLAIN, size=70, replace=False)
    specials = (ZERO, NAN_ROW, PINF_ROW, NINF_ROW)
    lists, dists = [], []
    for s in specials:
        for t in specials:
            lists.append(np.concatenate([[s], mid[:61], [t, NAN_ROW if s != NAN_ROW else ZERO]]))  # 64 positions
            dd = _dists(env, 64)
            if len(lists) % 3 == 0:
                dd[-1] = np.nan  # a NaN list distance, as the search reports for a NaN row
            if len(lists) % 5 == 0:
                dd[0] = np.inf
            dists.append(dd)
    lists.append(np.array(list(specials) * 3))
    dists.append(np.array([np.nan] * 4 + [np.inf] * 4 + [0.0, -0.0, 1.0, np.nan], dtype=np.float32))
    for lam in LAMBDAS:
        for k in (64, 5):
            _check(env, lists, dists, 64, k, lam, what=("specials", lam, k))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == 4], ids=lambda s: s[1])
def test_longest_list(shape):
    """ld = 4096 (every thread walks 16 positions; ids repeat, the index has fewer rows), k = 8, dim 4; one of the counts is shorter"""
    if shape not in _envs:
        _envs[shape] = Env(*shape)
    env, ld = _envs[shape], 4096
    lists = [env.rng.choice(PLAIN, size=ld), env.rng.choice(PLAIN, size=ld - 257)]
    dists = [_dists(env, ld), _dists(env, ld - 257)]
    for lam in (0.0, 0.5):
        _check(env, lists, dists, ld, 8, lam, what=("longest", lam))


def test_counts_are_clipped(env):
    """a count above ld reads ld entries; entries past a count are not read (they hold ids of no row)"""
    lists = [env.rng.choice(PLAIN, size=n, replace=False) for n in (70, 70, 3)]
    dists = [_dists(env, n) for n in (70, 70, 3)]
    got = _run(env.ix, lists, dists, 70, 70, 0.5, counts=[1000, 70, 3])
    exp = R.expect(env.rd, lists, dists, [70, 70, 3], 70, 0.5)
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32))


def test_id_offset(env):
    env.ix.set_id_offset(1 << 33)
    try:
        lists = [env.rng.choice(PLAIN, size=n, replace=False) for n in (129, 64)]
        gi, _, gc = _check(env, lists, [_dists(env, 129), _dists(env, 64)], 129, 100, 0.5, id_offset=1 << 33)
        assert (gi[0, :int(gc[0])] >= np.uint64(1 << 33)).all()
    finally:
        env.ix.set_id_offset(0)


def test_refusals_leave_outputs_and_counters(env):
    import lab_1806_vec_db_amd as vdb

    ix = env.ix
    stats = ("flat_mmr_calls", "flat_mmr_queries", "flat_fallback", "flat_i8_queries", "flat_filtered_queries")
    before = {s: ix.get_stat(s) for s in stats}
    untouched = lambda: (_run.last[0] == SENT).all() and (_run.last[1] == -7.0).all() and (_run.last[2] == SENT).all()  # noqa: E731
    for bad, off in ((N, 0), (1 << 40, 0), (5, 1000)):  # the first id past the rows; far past; below id_offset
        ix.set_id_offset(off)
        try:
            lists = [np.arange(10) + off, np.array([1 + off, 2 + off, bad, 3 + off])]  # (the ids as passed: id_offset included)
            with pytest.raises(vdb.VdbError, match="no row"):
                _run(ix, lists, [_dists(env, 10), _dists(env, 4)], 10, 5, 0.5)
            assert untouched()
        finally:
            ix.set_id_offset(0)
    one = [np.arange(4)], [_dists(env, 4)]
    for ld, k, lam in ((4, 2, float("nan")), (4, 2, -0.01), (4, 2, 1.5), (4, 2, float("inf")), (4, 5, 0.5), (4097, 2, 0.5)):
        with pytest.raises(vdb.VdbError, match="mmr"):
            _run(ix, one[0], one[1], ld, k, lam)
        assert untouched()
    u8 = vdb.GpuIndex(env.base.shape[1], "l2sqr", scalar="u8")
    try:
        u8.batch_add_u8(np.arange(8 * env.base.shape[1], dtype=np.uint8).reshape(8, -1))
        with pytest.raises(vdb.VdbError, match="f32 rows"):
            _run(u8, one[0], one[1], 4, 2, 0.5)
        assert untouched()
    finally:
        u8.close()
    assert before == {s: ix.get_stat(s) for s in stats}
    _check(env, one[0], one[1], 4, 2, 0.5)  # the index still answers
    assert before == {s: ix.get_stat(s) for s in stats}  # (the selection alone counts nothing)


def test_bad_id_text_and_the_call_after_it():
    """64 rows x dim 8, lists [2][4] with an id equal to len + id_offset, an id below id_offset, and both: the call raises with the exact
    text, the outputs keep their sentinel, and the valid call that follows on the same index is answered -- the flag word of the id check
    is zeroed by every call"""
    import re

    import lab_1806_vec_db_amd as vdb

    env = Env(8, "l2sqr", 0, base=np.random.default_rng(5).standard_normal((64, 8)).astype(np.float32))
    off = 1000
    env.ix.set_id_offset(off)
    try:
        good = [np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7])]
        dists = [_dists(env, 4), _dists(env, 4)]
        text = "mmr select: a list holds an id that is no row of this index (id - id_offset must be below len)"
        for past, below in ((True, False), (False, True), (True, True)):
            lists = [g + off for g in good]  # (the ids as passed: id_offset included)
            if past:
                lists[0][2] = 64 + off
            if below:
                lists[1][1] = off - 1
            with pytest.raises(vdb.VdbError, match=re.escape(text)):
                _run(env.ix, lists, dists, 4, 2, 0.5)
            assert (_run.last[0] == SENT).all() and (_run.last[1] == -7.0).all() and (_run.last[2] == SENT).all()
            _, _, gc = _check(env, good, dists, 4, 2, 0.5, id_offset=off, what=("after", past, below))
            assert gc.tolist() == [2, 2]
    finally:
        env.ix.close()
