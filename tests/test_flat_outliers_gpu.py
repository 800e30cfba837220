"""GPU: the k-NN self-join and the outlier scores end to end (GpuIndex.knn_graph / outliers and their device forms) against the oracle's pair
distances: the graph bit for bit with the row itself taken out by id, the scores against tests/lof_ref.py at its tolerance."""
import os

import numpy as np
import pytest
import torch

import lab_1806_vec_db_amd as vdb
import lof_ref as R
from test_flat_dups_gpu import _full_order, _index

pytestmark = pytest.mark.gpu
K, PLANTED = 20, [13, 77, 150, 222, 299]


@pytest.fixture(scope="module", params=(("l2sqr", 0), ("cosine", 1)), ids=("l2sqr", "cosine"))
def tables(request):
    """planted, 300 x 20: a cloud around one direction and five rows far from it in both metrics.  edges, 130 x 64: a zero row (under cosine at distance 1
    from itself and from every row), a NaN row (its distance to itself is NaN), three identical rows (the lower-index ones precede the row itself)"""
    dist, kind = request.param
    rng = np.random.default_rng(5)
    p = (2.0 + 0.3 * rng.standard_normal((300, 20))).astype(np.float32)
    p[PLANTED] = (-2.0 + 5.0 * np.eye(20)[:5] + 0.3 * rng.standard_normal((5, 20))).astype(np.float32)
    e = np.random.default_rng(6).standard_normal((130, 64)).astype(np.float32)
    e[100], e[40], e[[3, 77, 129]] = 0.0, np.nan, e[77]
    return dist, {name: (x, _full_order(x, kind)) for name, x in (("planted", p), ("edges", e))}


def _check(ix, full, k, allowed=None, id_offset=0):
    """knn_graph and outliers of `ix` against the reference over the oracle's order; returns (rows, the reference's lof, the library's)"""
    rows, nbr, nd, cnt = R.graph_of_order(*full, k, allowed)
    mask = None if allowed is None else ix.make_mask(allowed)
    ids, dists, counts = ix.knn_graph(k, mask)
    used = np.arange(k)[None, :] < cnt[:, None]
    assert np.array_equal(counts, cnt) and np.array_equal(ids, np.where(used, rows[nbr] + id_offset, 0))
    assert np.array_equal(dists.view(np.uint32), np.where(used, nd, np.float32(0)).view(np.uint32))  # bit for bit, zeros behind the count
    want, got = R.of_lists(nbr, nd, cnt), ix.outliers(k, mask)
    assert np.array_equal(got[0], want[0], equal_nan=True)
    R.close(got[1], want[1]), R.close(got[2], want[2])
    if mask is not None:
        mask.close()
    return rows, want[2], got[2]


@pytest.mark.parametrize("name,k", (("planted", K), ("planted", 100), ("edges", K), ("edges", 70), ("edges", 128)))  # 64 < k + 1: more than one tile of the pack walk
def test_graph_and_scores_at_every_chunk_size(tables, name, k):
    dist, (x, full) = tables[0], tables[1][name]
    ix = _index(dist, x)
    for chunk, chunks in ((64, -(-len(x) // 64)), (100, -(-len(x) // 100)), (16384, 1)):
        before = [ix.get_stat(s) for s in ("flat_knn_graph_calls", "flat_knn_graph_chunks")]
        ix.set_param("flat_dup_chunk", chunk)
        rows, lof, got = _check(ix, full, k)
        assert [ix.get_stat(s) - b for s, b in zip(("flat_knn_graph_calls", "flat_knn_graph_chunks"), before)] == [2, 2 * chunks]
    if name == "planted" and k == K:  # the planted rows are the five highest scores -- a property of the table, so asserted on the reference first
        assert sorted(np.argsort(-lof)[:5].tolist()) == PLANTED and sorted(np.argsort(-got)[:5].tolist()) == PLANTED
    elif name == "edges":  # (conditions on the input) the NaN row stands at its index in its own order; under cosine the zero row at 99, behind 99 ties: absent from
        oi = full[0]  # its own k + 1 nearest at k = 20 and 70 (the last entry dropped, in tile 1 at 70), in tile 1 at k = 128; a duplicate ahead of self
        assert oi[40].tolist().index(40) == 40 and (dist != "cosine" or oi[100].tolist().index(100) == 99) and oi[77][:3].tolist() == [3, 77, 129] and np.isnan(lof[40])
    ix.close()


def test_the_counters_of_the_unmasked_search_underneath():
    """the 1000 x 960 golden rows forced onto the matrix tiers, whose 8-bit first pass counts its queries: every row is one, once per walk"""
    base = np.fromfile(os.path.join(os.path.dirname(__file__), "golden", "gist_1000.bin"), dtype=np.float32).reshape(1000, 960)
    ix = _index("l2sqr", base, mode=2)
    ids, dists, counts = ix.knn_graph(10)
    assert ix.get_stat("flat_i8_queries") == 1000 and (counts == 10).all()
    ix.close()


def test_small_tables_a_mask_and_the_device_form(tables):
    dist, (x, full) = tables[0], tables[1]["edges"]
    for n in (1, 2, K, K + 1):  # m = 1: no neighbour, all NaN; m <= k: every other row is a neighbour
        sub = _index(dist, x[:n])
        _check(sub, (full[0][:n][full[0][:n] < n].reshape(n, n), full[1][:n][full[0][:n] < n].reshape(n, n)), K)
        sub.close()
    ix = _index(dist, x)
    ix.set_id_offset(1 << 33)
    allowed = np.arange(130) % 3 != 1  # (row 40 is outside, rows 3, 77, 129 and 100 inside)
    before = ix.get_stat("flat_filtered_queries")
    rows = _check(ix, full, 5, allowed, id_offset=1 << 33)[0]  # = the reference run on the sub-table: graph_of_order keeps the allowed rows only
    assert ix.get_stat("flat_filtered_queries") - before == 2 * len(rows)  # the masked search underneath, once per graph walk
    one = ix.make_mask(np.arange(130) == 100)
    assert ix.knn_graph(3, one)[2].tolist() == [0] and all(np.isnan(o).all() and o.shape == (1,) for o in ix.outliers(3, one))
    # the device forms; any score output may be left out
    m = int(allowed.sum())
    t_ids, t_d, t_c = (torch.full(s, -7, dtype=d, device="cuda") for s, d in (((m, 5), torch.int64), ((m, 5), torch.float32), ((m,), torch.int64)))
    t_lof = torch.full((m + 1,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mask = ix.make_mask(allowed)
    ix.knn_graph_device(5, t_ids.data_ptr(), t_d.data_ptr(), t_c.data_ptr(), mask)
    ix.outliers_device(5, 0, 0, t_lof.data_ptr(), mask)
    h_ids, h_d, h_c = ix.knn_graph(5, mask)
    assert np.array_equal(t_ids.cpu().numpy().view(np.uint64), h_ids) and np.array_equal(t_d.cpu().numpy(), h_d, equal_nan=True) and np.array_equal(t_c.cpu().numpy(), h_c.view(np.int64))
    assert np.array_equal(t_lof.cpu().numpy()[:m], ix.outliers(5, mask)[2], equal_nan=True) and t_lof.cpu().numpy()[m] == -7.0
    # every refusal leaves the outputs and the counters alone
    other, u8 = _index(dist, x[:50]), _index("l2sqr", np.ones((9, 64), dtype=np.uint8), u8=True)
    foreign, names = other.make_mask(np.ones(50, dtype=bool)), ("flat_knn_graph_calls", "flat_knn_graph_chunks", "flat_filtered_queries")
    before = [ix.get_stat(s) for s in names]
    t_lof.fill_(-7.0), torch.cuda.synchronize()
    for target, args, word in ((ix, (0, 0, 0, t_lof.data_ptr()), "k must be"), (ix, (1024, 0, 0, t_lof.data_ptr()), "k must be"),
                               (ix, (5, 0, 0, t_lof.data_ptr(), foreign), "another index"), (u8, (5, 0, 0, t_lof.data_ptr()), "f32 rows")):
        with pytest.raises(vdb.VdbError, match=word):
            target.outliers_device(*args)
    ix.batch_add(x[:1])
    with pytest.raises(vdb.VdbError, match="stale"):
        ix.outliers_device(5, 0, 0, t_lof.data_ptr(), mask)
    assert (t_lof.cpu().numpy() == -7.0).all() and [ix.get_stat(s) for s in names] == before
    for h in (foreign, one, mask, ix, other, u8):
        h.close()
