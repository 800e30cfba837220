"""GPU: the host forms of the Flat k-NN calls across the 16384-query chunk boundary of the shared host front end (csrc/api.hip:
host_search) -- flat_knn, flat_knn_filtered, flat_knn_filtered_multi and flat_knn_grouped with 16385 queries, so that the second chunk
is ONE query whose mask differs from the first query's.

64 rows of dimension 8, k = 3.  The queries repeat 32 distinct vectors; the oracle's full order (oracle.flat_knn_batch over all rows)
is computed for the 32 and tiled.  Two masks, even and odd rows; mask_of[q] = q & 1, and mask_of[16384] = 1: the queries on both sides
of the boundary use mask 1 and query 0 uses mask 0, so a chunk that read mask_of from its start instead of from q0 would answer the last
query under the wrong mask.  Every comparison is bit-exact (ids, distances as f32 bit patterns, counts), with the expectation helpers of
tests/test_flat_filtered_multi_gpu.py and tests/test_flat_grouped_gpu.py.  The counters a call moves are compared with literals: what
the same calls moved before the entry points shared host_search."""
import numpy as np
import pytest

from test_flat_filtered_multi_gpu import _expect_knn, _full_order, _same_knn
from test_flat_grouped_gpu import _expect as _expect_grouped

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
N, DIM, K, NQ, DISTINCT = 64, 8, 3, 16385, 32
STATS = ("flat_filtered_queries", "flat_filtered_multi_calls", "flat_grouped_calls")
COLUMN = 2
# what the grouped call moves: its list calls go through the mask-per-query search, one per chunk and round (under L2Sqr the 512
# copies of one vector in the first chunk need a second round)
GROUPED_MOVED = {"l2sqr": (16897, 3, 1), "cosine": (16385, 2, 1)}


@pytest.fixture(scope="module")
def world():
    """rows, the 32 distinct query vectors, both metrics' full orders of the 32, masks' allow-lists, mask_of, labels (never changed)"""
    rng = np.random.default_rng(16385)
    base = rng.standard_normal((N, DIM)).astype(np.float32)
    q32 = rng.standard_normal((DISTINCT, DIM)).astype(np.float32)
    fulls = {kind: _full_order(base, q32, kind) for _, kind in DISTS}
    allows = [np.arange(N) % 2 == 0, np.arange(N) % 2 == 1]
    mask_of = (np.arange(NQ) & 1).astype(np.uint32)
    mask_of[16384] = 1
    assert mask_of[0] == 0 and mask_of[16383] == 1 and mask_of[16384] == 1
    labels = ((np.arange(N) // 2) % 4).astype(np.uint32)  # 4 values, each under both masks
    return base, q32, fulls, allows, mask_of, labels


def _tile(per_mask, mask_of):
    """the expectation of the NQ queries from those of the 32 distinct vectors under each mask: query q is vector q % 32 under mask_of[q]"""
    v = np.arange(NQ) % DISTINCT
    return tuple(np.stack([e[j] for e in per_mask])[mask_of, v] for j in range(3))


def _index(dist, base, labels):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(DIM, dist)
    ix.batch_add(base)
    ix.set_labels(COLUMN, labels)
    return ix


def _run(ix, call):
    s0 = [ix.get_stat(s) for s in STATS]
    got = call()
    moved = tuple(ix.get_stat(s) - v for s, v in zip(STATS, s0))
    print("counters moved", dict(zip(STATS, moved)))
    return got, moved


@pytest.mark.parametrize("dist,kind", DISTS)
def test_host_calls_across_the_chunk_boundary(world, dist, kind):
    base, q32, fulls, allows, mask_of, labels = world
    full = fulls[kind]
    qs = np.ascontiguousarray(q32[np.arange(NQ) % DISTINCT])
    zeros = np.zeros(NQ, dtype=np.uint32)
    ix = _index(dist, base, labels)
    try:
        masks = [ix.make_mask(a) for a in allows]
        # flat_knn itself
        got, moved = _run(ix, lambda: ix.flat_knn(qs, K))
        _same_knn(got, _tile([_expect_knn(full, np.ones(N, dtype=np.bool_), K)], zeros), (dist, "flat_knn"))
        assert moved == (0, 0, 0), moved
        # one mask
        got, moved = _run(ix, lambda: ix.flat_knn_filtered(qs, K, masks[0]))
        _same_knn(got, _tile([_expect_knn(full, allows[0], K)], zeros), (dist, "filtered"))
        assert moved == (16385, 0, 0), moved
        # one mask per query
        got, moved = _run(ix, lambda: ix.flat_knn_filtered_multi(qs, K, masks, mask_of))
        exp = _tile([_expect_knn(full, a, K) for a in allows], mask_of)
        _same_knn(got, exp, (dist, "filtered_multi"))
        assert not np.array_equal(exp[0][16384], exp[0][0])  # (the boundary query's answer is not the one mask_of[0] would give)
        assert moved == (16385, 1, 0), moved
        # grouped, one hit per label value, under those masks
        got, moved = _run(ix, lambda: ix.flat_knn_grouped(qs, K, COLUMN, 1, masks, mask_of))
        m32 = [np.full(DISTINCT, g, dtype=np.uint32) for g in (0, 1)]
        _same_knn(got, _tile([_expect_grouped(full, labels, K, 1, allows, m) for m in m32], mask_of), (dist, "grouped"))
        assert moved == GROUPED_MOVED[dist], moved
        for m in masks:
            m.close()
    finally:
        ix.close()
