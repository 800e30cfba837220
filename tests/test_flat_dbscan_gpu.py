"""GPU: the density clustering end to end (GpuIndex.dbscan / dbscan_device) against tests/dbscan_ref.py over the oracle's pair distances."""
import numpy as np
import pytest
import torch

import dbscan_ref as R
import dup_ref
import lab_1806_vec_db_amd as vdb
from test_flat_dups_gpu import _full_order, _index  # (an index over a table; the oracle's full order of every row against every row)

pytestmark = pytest.mark.gpu
N, DIM, MIN_SAMPLES = 300, 20, 8


@pytest.fixture(scope="module")
def small():
    """(table, {kind: (the oracle's distance matrix, eps: 12 neighbours per row on average)}); three blobs interleaved with scattered rows"""
    rng, blob = np.random.default_rng(77), np.arange(N) % 10 < 7
    x = np.where(blob[:, None], np.eye(3, DIM)[np.arange(N) % 3] * 4 + rng.standard_normal((N, DIM)) * 0.12, rng.standard_normal((N, DIM)) * 2).astype(np.float32)
    x[[5, 17, 150, 299]], x[[64, 191]], x[200] = x[5], x[64], np.nan
    out = {kind: np.empty((N, N), dtype=np.float32) for kind in (0, 1)}
    for kind, D in out.items():
        np.put_along_axis(D, *_full_order(x, kind), axis=1)
    return x, {kind: (D, float(np.sort(D[np.isfinite(D)])[12 * N])) for kind, D in out.items()}


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_blobs_chunks_counters_device_form_and_refusals(small, dist, kind):
    x, (D, eps) = small[0], small[1][kind]
    exp = R.of_matrix(D, eps, MIN_SAMPLES)
    assert exp[2]["clusters"] >= 2 and min(exp[2][k] for k in ("core", "border", "noise")) >= 1 and exp[1][200] == 1  # conditions on the input; the NaN row is noise
    ix, other = _index(dist, x), _index(dist, x[:200])
    for chunk, chunks in ((64, 5), (100, 3), (16384, 1)):  # the same bits at every chunk size, and the counters
        before = [ix.get_stat(s) for s in R.COUNTERS]
        ix.set_param("flat_dup_chunk", chunk)
        R.same(ix.dbscan(eps, MIN_SAMPLES), exp)
        assert [ix.get_stat(s) - b for s, b in zip(R.COUNTERS, before)] == [1, chunks, exp[2]["pairs"]]
    R.same(ix.dbscan(0.0, 2), R.of_matrix(D, 0.0, 2))  # identical rows at eps = 0
    if kind == 0:  # ... two clusters of core rows, everything else noise; and min_samples = 1 on a NaN-free table is dup_groups
        assert ix.dbscan(0.0, 2)[2] == {"clusters": 2, "core": 6, "border": 0, "noise": N - 6, "pairs": 14} and np.array_equal(other.dbscan(eps, 1)[0], other.dup_groups(eps)[0])
    ix.set_id_offset(1 << 33)  # the device form, with an id offset
    lab, knd = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((N + 1,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ix.dbscan_device(eps, MIN_SAMPLES, lab.data_ptr(), knd.data_ptr())  # (returns synchronised)
    R.same((lab.cpu().numpy().view(np.uint64)[:N], knd.cpu().numpy()[:N], st), R.of_matrix(D, eps, MIN_SAMPLES, id_offset=1 << 33))
    # every refusal leaves the outputs (refilled with sentinels) and the counters alone
    foreign, stale, before = other.make_mask(np.ones(200, dtype=bool)), ix.make_mask(np.ones(N, dtype=bool)), [ix.get_stat(s) for s in R.COUNTERS]
    ix.batch_add(x[:1])  # (the mask made before it is stale now; the outputs hold N + 1 rows)
    lab.fill_(-7), knd.fill_(9), torch.cuda.synchronize()
    for args, word in (((float("nan"), 5, lab.data_ptr(), knd.data_ptr()), "NaN"), ((eps, 0, lab.data_ptr(), knd.data_ptr()), "min_samples"),
                       ((eps, 2**32, lab.data_ptr(), knd.data_ptr()), "min_samples"), ((eps, 5, lab.data_ptr(), knd.data_ptr(), foreign), "another index"),
                       ((eps, 5, lab.data_ptr(), knd.data_ptr(), stale), "stale"), ((eps, 5, 0, knd.data_ptr()), "null"),
                       ((eps, 5, lab.data_ptr(), 0), "null")):
        with pytest.raises(vdb.VdbError, match=word):
            ix.dbscan_device(*args)
    assert (lab.cpu().numpy() == -7).all() and (knd.cpu().numpy() == 9).all() and [ix.get_stat(s) for s in R.COUNTERS] == before
    for h in (foreign, stale, ix, other):
        h.close()


@pytest.mark.parametrize("dtype", (np.float32, np.uint8))
def test_a_masked_row_does_not_bridge_two_clusters(dtype):
    """a chain at squared distance 1 and two rows far away, on an f32 and on a u8 index; then without row 3"""
    y = np.zeros((9, DIM), dtype=dtype)
    y[:, 1] = [0, 1, 2, 3, 4, 5, 6, 100, 200]
    ix = _index("l2sqr", y, u8=dtype == np.uint8)
    lab, knd, st = ix.dbscan(1.0, 3)
    assert lab.tolist() == [1] * 7 + [R.ROW_NOISE] * 2 and knd.tolist() == [2, 3, 3, 3, 3, 3, 2, 1, 1] and st["pairs"] == 12
    lab, knd, st = ix.dbscan(1.0, 3, mask=ix.make_mask(np.arange(9) != 3))
    assert lab.tolist() == [1, 1, 1, R.ROW_NONE, 5, 5, 5, R.ROW_NOISE, R.ROW_NOISE] and knd.tolist() == [2, 3, 2, 0, 2, 3, 2, 1, 1] and st["pairs"] == 8
    ix.close()


def test_planted_table_on_the_8_bit_range_tier():
    """test_flat_dups_gpu's 20 000 x 128 table.  The reference lists are the library's own range_search results: this case tests the stage behind the join and
    the tier routing, not the distances; every planted pair lies inside half the radius in float64 (here), every other outside twice it (test_dup_ref_cpu)."""
    x, radius, _, pairs, _ = dup_ref.planted_table(20000, 128, "f32", dup_ref.PLANTED_SEEDS["f32"])
    assert (((x[pairs[:, 0]].astype(np.float64) - x[pairs[:, 1]]) ** 2).sum(axis=1) * 2 <= radius).all()
    ix = _index("l2sqr", x, mode=2)
    exp = R.dbscan_ref(len(x), list(range(len(x))), *ix.range_search(x, radius), 3)
    assert exp[2]["clusters"] >= 50 and exp[2]["border"] >= 1 and exp[2]["pairs"] == 2 * len(pairs)
    i8 = ix.get_stat("flat_range_i8_queries")
    R.same(ix.dbscan(radius, 3), exp)
    assert ix.get_stat("flat_range_i8_queries") > i8  # the tier ran
    ix.close()
