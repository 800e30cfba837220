"""GPU: the stage behind the self-join alone (GpuIndex.dbscan_pairs_device; k_dbscan.hip) over hand-made symmetric CSR lists, bit for bit."""
import numpy as np
import pytest
import torch

import dbscan_ref as R
import lab_1806_vec_db_amd as vdb
from test_flat_dups_gpu import _index

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    made = {n: _index("l2sqr", np.ones((n, 4), dtype=np.float32)) for n in (1, 63, 64, 65, 5000)}  # (the rows are never looked at)
    yield made
    for ix in made.values():
        ix.close()


def _run(ix, src, lists, min_samples, id_offset=0, lims=None, check=False):
    """-> (label, kind, stats), sentinel-filled outputs kept in _run.last even when the call raises; min_samples None: link_pairs_device;
    check: compared with the reference"""
    l_, i_, d_ = R.csr(lists)
    arrays = (np.asarray(src, dtype=np.uint64) + np.uint64(id_offset), l_ if lims is None else np.asarray(lims, dtype=np.uint64), i_ + np.uint64(id_offset))
    t = [torch.from_numpy(np.concatenate([a, np.zeros(1, dtype=np.uint64)]).view(np.int64)).cuda() for a in arrays]  # (never an empty tensor)
    t += [torch.from_numpy(np.concatenate([d_, np.zeros(1, dtype=np.float32)])).cuda()]
    lab, knd = torch.full((len(ix),), -7, dtype=torch.int64, device="cuda"), torch.full((len(ix),), 9, dtype=torch.uint8, device="cuda")
    ix.set_id_offset(id_offset)
    torch.cuda.synchronize()
    try:
        if min_samples is None:
            return lab, None, ix.link_pairs_device(*(x.data_ptr() for x in t[:3]), len(src), lab.data_ptr())
        stats = ix.dbscan_pairs_device(*(x.data_ptr() for x in t), len(src), min_samples, lab.data_ptr(), knd.data_ptr())
    finally:
        ix.set_id_offset(0)
        _run.last = lab.cpu().numpy().view(np.uint64), knd.cpu().numpy()
    if check:
        R.same(_run.last + (stats,), R.dbscan_ref(len(ix), src, l_, i_, d_, min_samples, id_offset=id_offset))
    return _run.last + (stats,)


@pytest.mark.parametrize("id_offset", (0, 1 << 40))
@pytest.mark.parametrize("name,n,min_samples,edges,label,kind", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_cases(tables, name, n, min_samples, edges, label, kind, id_offset):
    lab, knd, _ = _run(tables[65], *R.lists_of_edges(n, edges), min_samples, id_offset, check=True)
    assert lab[:n].tolist() == [v if v >= R.ROW_NOISE else v + id_offset for v in label] and (lab[n:] == R.ROW_NOISE).all()
    assert knd[:n].tolist() == kind and (knd[n:] == 1).all()  # the rows behind the case are no source: an empty neighbourhood, noise


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_table_sizes(tables, n):
    _run(tables[n], *R.lists_of_edges(n, [(i, i + 1, 1) for i in range(n - 1)]), 3, check=True)  # a path of core rows, a border row at each end
    _run(tables[n], *R.lists_of_edges(n, [(0, k, k) for k in range(1, n)]), n, check=True)  # a star: min_samples = leaves + 1
    _, knd, st = _run(tables[n], list(range(n)), [[]] * n, 1, check=True)  # empty lists
    assert (knd == 1).all() and st == dict.fromkeys(R.STATS, 0) | {"noise": n}


@pytest.mark.parametrize("length,at", ((64, 63), (65, 63), (65, 64), (129, 63), (129, 64)))
def test_the_deciding_core_neighbour_at_a_tile_boundary(tables, length, at):
    """the only core row of row 0's list at position `at` (lane 63, or lane 0 of the next tile); it is core through rows 1000 .. of its own"""
    edges = [(0, k, k) for k in range(1, length)] + [(at, 1000 + k, 0.5) for k in range(length - 1)]
    lab, knd, st = _run(tables[5000], *R.lists_of_edges(1000 + length, edges), length + 1, check=True)
    assert lab[0] == at and knd[0] == 2 and knd[at] == 3 and st["clusters"] == 1 and st["core"] == 1 and st["border"] == length


def test_geometric_graph_two_calls_and_link_pairs(tables):
    p = np.random.default_rng(11).random((5000, 2), dtype=np.float32)  # a random geometric graph: about 9 rows within the radius of each
    dx, dy = p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]
    src, lists = R.lists_of_matrix(dx * dx + dy * dy, 9.0 / (5000 * np.pi))
    mid = _run(tables[5000], src, lists, 8, check=True)
    assert mid[2]["clusters"] >= 2 and min(mid[2][k] for k in ("core", "border", "noise")) > 0  # (a condition on the input)
    R.same(_run(tables[5000], src, lists, 8), mid)  # the same bits from two calls
    one = _run(tables[5000], src, lists, 1, check=True)  # min_samples = 1: every row is core, and the clusters are link_pairs_device's groups
    _run(tables[5000], src, lists, None)
    assert (one[1] == 3).all() and np.array_equal(one[0], _run.last[0])


@pytest.mark.parametrize("kw", (dict(lists=[[(1, 1.0), (65, 2.0)], [(0, 1.0)]]), dict(lims=[0, 2, 1]), dict(lims=[1, 2, 3]), dict(src=[0, 65]),
                                dict(src=[1, 1]), dict(min_samples=0), dict(min_samples=2**32)), ids=str)
def test_refusals_leave_outputs_and_counters_alone(tables, kw):
    """an id or a source that is no row, limits that descend or do not start at 0, a source named twice, min_samples outside 1 .. 2^32 - 1"""
    before = [tables[65].get_stat(s) for s in R.COUNTERS]
    kw = {"src": [0, 1], "lists": [[(1, 1.0), (2, 2.0)], [(0, 1.0)]], "min_samples": 2, **kw}
    with pytest.raises(vdb.VdbError, match="dbscan"):
        _run(tables[65], **kw)
    assert (_run.last[0] == np.uint64(2**64 - 7)).all() and (_run.last[1] == 9).all() and [tables[65].get_stat(s) for s in R.COUNTERS] == before
