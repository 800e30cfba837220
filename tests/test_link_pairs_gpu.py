"""GPU: the component stage alone (GpuIndex.link_pairs_device, vdb_link_pairs_device; k_components.hip) over hand-made CSR edge lists
against tests/dup_ref.py, with exact equality of `group` and `stats`.  The lists are taken as given -- any ids, any order, repeats -- so
the expected answer is dup_ref over the same lists: the lowest row of every component, whatever order the waves hooked the roots in."""
import numpy as np
import pytest

import dup_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 5000)
SENT = -7


@pytest.fixture(scope="module")
def tables():
    """one index per table size (dim 4; the rows are never looked at), and one of 200 000 rows"""
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(5)
    made = {}
    for n in SIZES + (200_000,):
        ix = vdb.GpuIndex(4, "l2sqr", device=0)
        ix.batch_add(rng.random((n, 4), dtype=np.float32))
        made[n] = ix
    yield made
    for ix in made.values():
        ix.close()


def _run(ix, src, lists, id_offset=0, lims=None, ids=None):
    """-> (group uint64 [n], stats) from the device; the output is pre-filled with a sentinel and read back even when the call raises"""
    import torch

    n, nq = len(ix), len(src)
    l_, i_ = R.csr(lists)
    lims = l_ if lims is None else np.asarray(lims, dtype=np.uint64)
    ids = i_ + np.uint64(id_offset) if ids is None else np.asarray(ids, dtype=np.uint64)
    s = np.asarray(src, dtype=np.uint64) + np.uint64(id_offset)
    pad = lambda a: np.concatenate([a, np.zeros(1, dtype=np.uint64)])  # (never an empty tensor: its pointer would be null)
    t_src = torch.from_numpy(pad(s).view(np.int64)).cuda()
    t_lims = torch.from_numpy(pad(lims).view(np.int64)).cuda()
    t_ids = torch.from_numpy(pad(ids).view(np.int64)).cuda()
    out = torch.full((max(n, 1),), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        stats = ix.link_pairs_device(t_src.data_ptr(), t_lims.data_ptr(), t_ids.data_ptr(), nq, out.data_ptr())
    finally:
        torch.cuda.synchronize()
        _run.last = out.cpu().numpy().view(np.uint64)[:n]
    return _run.last, stats


def _check(ix, src, lists, id_offset=0, what=""):
    n = len(ix)
    lims, ids = R.csr(lists)
    eg, es = R.dup_ref(n, src, lims, ids, id_offset=id_offset)
    gg, gs = _run(ix, src, lists, id_offset)
    assert gs == es, (what, gs, es)
    assert np.array_equal(gg, eg), (what, np.flatnonzero(gg != eg)[:8])
    return gg, gs


def _shapes(n, rng):
    """(name, src, lists) over a table of n rows"""
    rows = list(range(n))
    yield "path", rows, [[i, i + 1] if i + 1 < n else [i] for i in rows]
    yield "reversed path", rows[::-1], [[i, i - 1] if i else [i] for i in rows[::-1]]
    yield "path from the far end, no self pairs", rows[:0:-1], [[i - 1] for i in rows[:0:-1]]
    yield "star on row 0", rows, [rows] + [[i] for i in rows[1:]]
    yield "star on the last row", rows, [[i] for i in rows[:-1]] + [rows[::-1]]
    yield "every row lists rows 0..7", rows, [[i] + [j for j in range(min(8, n))] for i in rows]
    c = min(300, n)
    yield "one clique", rows[:c], [rows[:c] for _ in range(c)]
    for dens in (0.3, 1.5):
        m = int(n * dens)
        u, v = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
        once = [[] for _ in rows]
        for a, b in zip(u.tolist(), v.tolist()):
            once[a].append(b)
        yield f"random sparse {dens} once", rows, once
        yield f"random sparse {dens} twice", rows, [x + x for x in once]
        both = [list(x) for x in once]
        for a, b in zip(u.tolist(), v.tolist()):
            both[b].append(a)
        yield f"random sparse {dens} both directions", rows, both
    yield "empty lists", rows, [[] for _ in rows]
    yield "self-only lists", rows, [[i] for i in rows]
    yield "no lists", [], []
    yield "one list with repeats, the rest missing", [n - 1], [[0, n - 1, 0, 0]]


@pytest.mark.parametrize("n", SIZES)
def test_shapes_against_the_reference(tables, n):
    ix = tables[n]
    rng = np.random.default_rng(100 + n)
    for name, src, lists in _shapes(n, rng):
        _check(ix, src, lists, what=(n, name))


def test_two_hundred_thousand_rows(tables):
    n = 200_000
    ix = tables[n]
    rng = np.random.default_rng(9)
    import torch

    def run(src, lims, ids):
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda() for a in (src, lims, ids)]
        out = torch.full((n,), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = ix.link_pairs_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(src), out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint64), st

    rows = np.arange(n, dtype=np.uint64)
    # the path of all rows, forward and reversed: one group, whatever depth the trees reach on the way
    for src in (rows, rows[::-1]):
        nxt = np.where(src + 1 < n, src + 1, src)
        g, st = run(src, np.arange(0, n + 1, dtype=np.uint64), nxt)
        assert not g.any() and st == {"groups": 1, "rows": n, "pairs": n - 1, "truncated": 0}
    # a random sparse graph against the reference (vectorised here: scipy-free label propagation would be slow at this size)
    m = n // 2
    u, v = rng.integers(0, n, size=m).astype(np.uint64), rng.integers(0, n, size=m).astype(np.uint64)
    order = np.argsort(u, kind="stable")
    u, v = u[order], v[order]
    src, counts = np.unique(u, return_counts=True)
    lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    eg, es = R.dup_ref(n, src.tolist(), lims, v)
    g, st = run(src, lims, v)
    assert st == es and np.array_equal(g, eg)
    g2, st2 = run(src, lims, v)
    assert st2 == st and np.array_equal(g2, g)  # the same call twice: the same bits


def test_id_offset(tables):
    ix = tables[257]
    rng = np.random.default_rng(3)
    ix.set_id_offset(1 << 40)
    try:
        for name, src, lists in _shapes(257, rng):
            g, _ = _check(ix, src, lists, id_offset=1 << 40, what=name)
            assert g.min() >= 1 << 40
    finally:
        ix.set_id_offset(0)


def test_the_same_call_twice_gives_the_same_bits(tables):
    ix = tables[5000]
    rng = np.random.default_rng(4)
    for name, src, lists in list(_shapes(5000, rng))[6:10]:
        a, sa = _run(ix, src, lists)
        b, sb = _run(ix, src, lists)
        assert sa == sb and np.array_equal(a, b), name


def test_refusals_leave_output_and_counters_alone(tables):
    import lab_1806_vec_db_amd as vdb

    ix = tables[65]
    n = 65
    names = ("flat_dup_calls", "flat_dup_chunks", "flat_dup_pairs", "flat_range_queries", "fetch_calls")
    before = [ix.get_stat(s) for s in names]
    sent = np.full(n, np.uint64(SENT & (2**64 - 1)))
    src, lists = [0, 1, 2], [[1, 2], [0], [2, 3, 4]]
    bad_calls = [
        dict(ids=[1, 2, 0, 2, 3, n]),                       # an id that is no row
        dict(ids=[1, 2, 0, 2, 3, 2**64 - 1]),
        dict(lims=[0, 2, 1, 6]),                            # limits that descend
        dict(lims=[1, 2, 3, 6]),                            # limits that do not start at 0
    ]
    for kw in bad_calls:
        with pytest.raises(vdb.VdbError, match="link pairs"):
            _run(ix, src, lists, **kw)
        assert np.array_equal(_run.last, sent), kw
    with pytest.raises(vdb.VdbError, match="link pairs"):   # a source id that is no row
        _run(ix, [0, n, 2], lists)
    assert np.array_equal(_run.last, sent)
    ix.set_id_offset(100)                                   # ids below the offset
    try:
        with pytest.raises(vdb.VdbError, match="link pairs"):
            _run(ix, src, lists, id_offset=0)
        assert np.array_equal(_run.last, sent)
    finally:
        ix.set_id_offset(0)
    import torch

    out = torch.full((n,), SENT, dtype=torch.int64, device="cuda")
    one = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for args in ((0, one.data_ptr(), one.data_ptr(), 1, out.data_ptr()), (one.data_ptr(), 0, one.data_ptr(), 1, out.data_ptr()),
                 (one.data_ptr(), one.data_ptr(), 0, 1, out.data_ptr()), (one.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 0),
                 (one.data_ptr() + 4, one.data_ptr(), one.data_ptr(), 1, out.data_ptr()), (one.data_ptr(), one.data_ptr(), one.data_ptr(), 2**32, out.data_ptr())):
        with pytest.raises(vdb.VdbError, match="link pairs"):
            ix.link_pairs_device(*args)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), sent)
    assert [ix.get_stat(s) for s in names] == before
    # ... and the stage alone moves none of the self-join's counters when it succeeds either
    _check(ix, src, lists)
    assert [ix.get_stat(s) for s in names] == before
