"""GPU: the sharded range search leaves no device memory behind -- create / set_rows / range / close cycles in both layouts, with and
without the 1-rank communicator and with three ranks on the one GPU (VDB_CTX_LOOPBACK=1), return all of it (hipMemGetInfo through torch); and at the ctypes level a vdb_range returned by
vdb_sharded_flat_range is still readable after vdb_sharded_destroy and gives its memory back on vdb_range_destroy."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sharded_range_cycles_return_all_memory(monkeypatch):
    torch = pytest.importorskip("torch")
    from lab_1806_vec_db_amd.sharded import ShardedIndex

    rng = np.random.default_rng(1)
    base = rng.standard_normal((20000, 64)).astype(np.float32)
    qs = rng.standard_normal((40, 64)).astype(np.float32)

    def cycle():
        for force in ("0", "1"):
            monkeypatch.setenv("VDB_CTX_FORCE_RCCL", force)
            sh = ShardedIndex(64, "l2sqr", devices=[0])
            sh.set_rows(base)
            lims, idx, dist = sh.range_search(qs, np.inf)  # 800 000 pairs: result, staging and receive buffers of ~10 MB each
            assert int(lims[-1]) == 40 * 20000
            sh.range_search(qs, np.inf, limit=7)
            sh.range_search(qs, 60.0)
            sh.close()
            sh = ShardedIndex(64, "l2sqr", devices=[0])
            sh.set_rows_replica(base[:3000])
            sh.range_search(qs, np.inf)
            sh.close()
        # three ranks on the one GPU through the loopback exchange: the phase-2 staging (send block, 3 x that to receive) of every shard
        monkeypatch.setenv("VDB_CTX_FORCE_RCCL", "0")
        monkeypatch.setenv("VDB_CTX_LOOPBACK", "1")
        sh = ShardedIndex(64, "l2sqr", devices=[0, 0, 0])
        sh.set_rows(base)
        lims, idx, dist = sh.range_search(qs, np.inf)
        assert int(lims[-1]) == 40 * 20000
        sh.range_search(qs, np.inf, limit=7)
        sh.close()
        sh = ShardedIndex(64, "l2sqr", devices=[0, 0, 0])
        sh.set_rows_replica(base[:3000])
        sh.range_search(qs, np.inf)
        sh.close()
        monkeypatch.delenv("VDB_CTX_LOOPBACK")

    cycle()  # first use: the runtime's own pools, the library's code objects, RCCL's
    gc.collect()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(8):
        cycle()
    gc.collect()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (64 << 20), (free0, free1)  # (the allocator keeps granules around; a leak of 8 cycles would be hundreds of MB)


def test_range_object_outlives_the_sharded_index():
    torch = pytest.importorskip("torch")
    from lab_1806_vec_db_amd import _lib as L

    lib = L.load()
    n, dim, nq = 20000, 64, 300  # 6 000 000 pairs: 72 MB in the result object
    rng = np.random.default_rng(2)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    radius = np.full(nq, np.inf, dtype=np.float32)
    devs = np.zeros(1, dtype=np.int32)
    ctx, sh, res = L.vp(), L.vp(), L.vp()
    torch.cuda.synchronize()
    L.check(lib.vdb_ctx_create(devs.ctypes.data_as(L.intp), 1, C.byref(ctx)))
    L.check(lib.vdb_sharded_create(ctx, dim, 0, C.byref(sh)))
    L.check(lib.vdb_sharded_set_rows(sh, base.ctypes.data_as(L.f32p), n))
    L.check(lib.vdb_sharded_flat_range(sh, qs.ctypes.data_as(L.f32p), nq, dim, radius.ctypes.data_as(L.f32p), 0, C.byref(res)))
    L.check(lib.vdb_sharded_destroy(sh))
    L.check(lib.vdb_ctx_destroy(ctx))
    free_with, _ = torch.cuda.mem_get_info()
    lims = np.zeros(nq + 1, dtype=np.uint64)
    L.check(lib.vdb_range_lims(res, lims.ctypes.data_as(L.u64p)))
    assert lims.tolist() == [q * n for q in range(nq + 1)]
    idx = np.zeros(nq * n, dtype=np.uint64)
    dist = np.zeros(nq * n, dtype=np.float32)
    L.check(lib.vdb_range_copy(res, idx.ctypes.data_as(L.u64p), dist.ctypes.data_as(L.f32p)))
    from oracle import oracle as O

    pick = [0, 137, nq - 1]
    oi, od, oc = O.flat_knn_batch(base, qs[pick], n, 0, nthreads=16)
    for j, q in enumerate(pick):  # what vdb_flat_range returns for an infinite radius: all rows in the reference's order
        assert np.array_equal(idx[q * n:(q + 1) * n], oi[j].astype(np.uint64))
        assert np.array_equal(dist[q * n:(q + 1) * n].view(np.uint32), od[j].view(np.uint32))
    L.check(lib.vdb_range_destroy(res))
    free_without, _ = torch.cuda.mem_get_info()
    assert free_without - free_with >= (48 << 20), (free_with, free_without)  # 72 MB of pairs went back
