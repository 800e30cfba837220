"""CPU rehearsal of the row-sharded range search's exchange (shard.allgather_merge_range) with the gloo backend, worlds 2 and 3.

Every rank derives its local CSR result from the CPU oracle on its own row block (global ids, standing in for GpuIndex.range_search
with set_id_offset), runs the product's two collectives + merge, and every rank's output must equal the oracle's UNSHARDED answer bit
for bit: for radii at the 10th distance (7 rows: the 3rd), just below it, NaN, +inf, and with limit = 3.  The last row is a copy of row 3, which
lies in the first shard: an exact distance tie between ranks in every case; with n = 7 the shards are uneven and +inf returns all 7 rows.
The replica exchange (allgather_concat_range) is rehearsed the same way."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

DIM, NQ = 24, 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _corpus(n):
    rng = np.random.default_rng(123)
    base = rng.standard_normal((n, DIM)).astype(np.float32)
    base[n - 1] = base[3]  # row 3 is in the first shard, row n - 1 in the last: an exact distance tie across ranks
    qs = rng.standard_normal((NQ, DIM)).astype(np.float32)
    return base, qs


def _full_order(base, qs):
    from oracle import oracle as O

    if len(base) == 0:
        return np.zeros((len(qs), 0), np.uint64), np.zeros((len(qs), 0), np.float32)
    oi, od, oc = O.flat_knn_batch(base, qs, len(base), 0)
    assert (oc == len(base)).all()
    return oi.astype(np.uint64), od


def _expect(full, radii, limit=None, id_offset=0):
    oi, od = full
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        with np.errstate(invalid="ignore"):
            inside = od[q] <= np.float32(radii[q])  # NaN radius: False
        cut = int(inside.sum())
        assert inside[:cut].all()
        if limit is not None:
            cut = min(cut, limit)
        ids.append(oi[q, :cut] + np.uint64(id_offset))
        ds.append(od[q, :cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(ids), np.concatenate(ds)


def _cases(full, n):
    kth = full[1][:, (3 if n == 7 else 10) - 1].copy()
    below = np.nextafter(kth, np.float32(-np.inf))
    nan = np.full(NQ, np.nan, dtype=np.float32)
    inf = np.full(NQ, np.inf, dtype=np.float32)
    return [("kth", kth, None), ("below", below, None), ("nan", nan, None), ("inf", inf, None), ("kth_limit3", kth, 3), ("inf_limit3", inf, 3)]


def _worker(rank, world, port, n, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lab_1806_vec_db_amd.shard import allgather_concat_range, allgather_merge_range, replica_query_slice, shard_bounds

        base, qs = _corpus(n)
        whole = _full_order(base, qs)  # only to derive the radii every rank uses
        r0, r1 = shard_bounds(n, world, rank)
        mine = _full_order(base[r0:r1], qs)
        q0, q1 = replica_query_slice(NQ, world, rank)
        out = {}
        for name, radii, limit in _cases(whole, n):
            ll, li, ld = _expect(mine, radii, limit, id_offset=r0)
            ml, mi, md = allgather_merge_range(torch.from_numpy(ll.astype(np.int64)), torch.from_numpy(li.astype(np.int64)),
                                               torch.from_numpy(ld), limit)
            out[name + "_lims"], out[name + "_idx"], out[name + "_dist"] = ml.numpy(), mi.numpy(), md.numpy()
            # replicas: this rank answers its query block on ALL rows
            bl, bi, bd = _expect((whole[0][q0:q1], whole[1][q0:q1]), radii[q0:q1], limit)
            cl, ci, cd = allgather_concat_range(torch.from_numpy(bl.astype(np.int64)), torch.from_numpy(bi.astype(np.int64)),
                                                torch.from_numpy(bd), NQ)
            out["rep_" + name + "_lims"], out["rep_" + name + "_idx"], out["rep_" + name + "_dist"] = cl.numpy(), ci.numpy(), cd.numpy()
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 501), (3, 100), (2, 7)])
def test_row_shard_range_exchange_equals_unsharded(tmp_path, world, n):
    port = _free_port()
    mp.spawn(_worker, args=(world, port, n, str(tmp_path)), nprocs=world, join=True)
    base, qs = _corpus(n)
    from lab_1806_vec_db_amd.shard import shard_bounds

    assert shard_bounds(n, world, 0)[1] > 3 and shard_bounds(n, world, world - 1)[0] <= n - 1 < shard_bounds(n, world, world - 1)[1] and world > 1
    whole = _full_order(base, qs)
    assert all(np.array_equal(whole[1][q][whole[0][q] == 3], whole[1][q][whole[0][q] == n - 1]) for q in range(NQ))  # the tie is there
    outs = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    for name, radii, limit in _cases(whole, n):
        el, ei, ed = _expect(whole, radii, limit)
        if name == "inf":
            assert el.tolist() == [q * n for q in range(NQ + 1)]  # every row of every shard, uneven shards included
        if name == "nan":
            assert int(el[-1]) == 0
        if name == "kth" and n != 7:
            assert int(el[-1]) >= 10 * NQ
        for o in outs:  # every rank holds the full merged answer
            for pre in ("", "rep_"):
                assert np.array_equal(o[pre + name + "_lims"].astype(np.uint64), el), (pre, name)
                assert np.array_equal(o[pre + name + "_idx"].astype(np.uint64), ei), (pre, name)
                assert o[pre + name + "_dist"].dtype == np.float32
                assert np.array_equal(o[pre + name + "_dist"].view(np.uint32), ed.view(np.uint32)), (pre, name)
