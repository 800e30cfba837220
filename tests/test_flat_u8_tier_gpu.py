"""GPU: Flat k-NN of a u8 table through the native 8-bit pass (k_gemm_u8.hip, "flat_u8" = 2) equals, bit for bit, an f32 twin index of the
widened rows and the oracle's u8 fold: 20 003 rows (a partially filled last tile), dims with a partial k-block (48), with exact L2Sqr keys
(128) and past them (272), one query and more than one group of 128, ties by index, zero vectors, queries the tier must hand on, row
edits, and the routing under auto."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NQ = 20003, 150
DISTS = [("l2sqr", 0), ("cosine", 1)]


@functools.lru_cache(maxsize=None)
def _pair(dist, kind, dim):
    """the u8 index (tier forced), its f32 twin, rows, queries and the oracle's first 100 (distance, row) pairs of three queries"""
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O

    rng = np.random.default_rng(dim + kind)
    base = rng.integers(0, 256, (N, dim), dtype=np.uint8)
    base[10000:10020] = base[:20]  # ties, decided by index
    base[77] = 0
    qs = rng.integers(0, 256, (NQ, dim), dtype=np.uint8)
    qs[0], qs[3] = base[7], 0
    u8, twin = vdb.GpuIndex(dim, dist, scalar="u8"), vdb.GpuIndex(dim, dist)
    u8.set_param("flat_u8", 2)
    u8.batch_add_u8(base)
    twin.batch_add(base.astype(np.float32))
    top = {q: sorted((np.float32(O.dist_u8(kind, r, qs[q])), i) for i, r in enumerate(base))[:100] for q in (0, 5, NQ - 1)}
    return u8, twin, base, qs, top


def _same(u8, twin, qs, k):
    got, want = u8.flat_knn_u8(qs, k), twin.flat_knn(qs.astype(np.float32), k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    return got


@pytest.mark.parametrize("nq", [1, NQ])
@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("dim", [48, 128, 272])
@pytest.mark.parametrize("dist,kind", DISTS)
def test_tier_equals_twin_and_oracle(dist, kind, dim, k, nq):
    u8, twin, base, qs, top = _pair(dist, kind, dim)
    before = u8.get_stat("flat_u8_queries")
    idx, d, _ = _same(u8, twin, qs[:nq], k)
    assert u8.get_stat("flat_u8_queries") == before + nq
    for q in (t for t in top if t < nq):
        assert idx[q].tolist() == [i for _, i in top[q][:k]] and d[q].tolist() == [x for x, _ in top[q][:k]], q


@pytest.mark.parametrize("dist,kind", DISTS)
def test_counters_handed_on_queries_edits_routing(dist, kind):
    import lab_1806_vec_db_amd as vdb

    dim = 128
    rng = np.random.default_rng(5 + kind)
    base = rng.integers(0, 256, (N, dim), dtype=np.uint8)
    qs = rng.integers(0, 256, (NQ, dim), dtype=np.uint8)
    u8, twin = vdb.GpuIndex(dim, dist, scalar="u8"), vdb.GpuIndex(dim, dist)
    u8.set_param("flat_u8", 2)
    u8.batch_add_u8(base)
    twin.batch_add(base.astype(np.float32))
    stat = u8.get_stat
    _same(u8, twin, qs, 10)
    assert stat("flat_u8_queries") == NQ and stat("flat_u8_valid") == 1
    # ... and an index only this tier has searched holds no mirror, only the 8 bytes of row constants
    assert stat("flat_half_valid") == 0 and stat("flat_bf16_mirror") == 0 and stat("hbm_bytes_per_row") <= dim + 4 + 8
    # one batch of eligible queries and four the tier must hand on: a fraction, 256, -1, NaN
    mixed = qs[:12].astype(np.float32)
    mixed[2, 5], mixed[4, 0], mixed[7, 127], mixed[9, 64] = 3.5, 256.0, -1.0, np.nan
    redo0 = stat("flat_u8_redo")
    got, want = u8.flat_knn(mixed, 10), twin.flat_knn(mixed, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    assert stat("flat_u8_redo") == redo0 + 4 and stat("flat_u8_queries") == NQ + 12
    # row edits: add (constants extended), swap_remove and remove_rows (constants dropped, rebuilt by the next search)
    extra = rng.integers(0, 256, (300, dim), dtype=np.uint8)
    u8.batch_add_u8(extra)
    twin.batch_add(extra.astype(np.float32))
    assert stat("flat_u8_valid") == 0
    _same(u8, twin, qs, 10)
    assert stat("flat_u8_valid") == 1
    for ix in (u8, twin):
        ix.swap_remove(5)
        ix.remove_rows(np.arange(19990, 20100))
    assert stat("flat_u8_valid") == 0
    _same(u8, twin, qs, 10)
    assert stat("flat_u8_valid") == 1
    # routing.  AS SHIPPED auto (0) engages for no shape -- every shape measured ran at 0.43 - 0.75 of the fp16 route's speed
    # (tools/bench_u8.py), and auto excludes a slower shape -- so the default, alone or with flat_half / flat_mode set, and "flat_u8" = 1
    # all keep today's path; 2 takes the tier again.  (The issue asked for a default index that takes the tier: not met, see the figures.)
    took = stat("flat_u8_queries")
    for u8_mode, name, value in ((0, None, 0), (0, "flat_half", 2), (0, "flat_mode", 2), (1, None, 0)):
        u8.set_param("flat_u8", u8_mode)
        if name:
            u8.set_flat_mode(value) if name == "flat_mode" else u8.set_param(name, value)
        _same(u8, twin, qs, 10)
        assert stat("flat_u8_queries") == took, (u8_mode, name)
        if name:
            u8.set_flat_mode(0) if name == "flat_mode" else u8.set_param(name, 0)
    u8.set_param("flat_u8", 2)
    _same(u8, twin, qs, 10)
    assert stat("flat_u8_queries") == took + NQ
