"""GPU: the device merges of per-shard k-NN lists on constructed inputs -- merge_topk_device, merge_topk_gathered and
merge_topk_gathered_async (k_merge_shards64 for k <= 64; k_pack_pairs + k_topk_merge<R> + k_finalize beyond) against the plain
reference of merge_ref.py, which test_merge_topk_cpu.py checks against the host merge on the same inputs.

One GPU stands in for S: the lists are built directly (merge_ref.flat_case), so they reach what search output cannot -- poison past
the counts, ties across shards under interleaved ids, NaN / -0 / inf / negative distances, shard order that is not id order, counts
above k, S*k around 64.  Bit-exact: ids, counts, distance bit patterns; every output is pre-filled with a sentinel."""
import functools

import numpy as np
import pytest

import merge_ref as M

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope="module")
def ix():
    import lab_1806_vec_db_amd as vdb

    x = vdb.GpuIndex(8, "l2sqr")
    yield x
    x.close()


@functools.lru_cache(maxsize=None)
def _case(S, k, nq):
    d, ids, counts = M.flat_case(S, nq, k, seed=1000 * S + k)
    return (d, ids, counts), M.merge_topk_ref(d, ids, counts, k)


def _dev(a):
    import torch

    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _outs(nq, k):
    import torch

    raw = [torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda") for n in (nq * k * 8, nq * k * 4, nq * 8)]
    return raw[0].view(torch.int64).view(nq, k), raw[1].view(torch.float32).view(nq, k), raw[2].view(torch.int64)


def _read(outs):
    return tuple(t.cpu().numpy() for t in outs)


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _merge_three_ways(ix, S, k, nq, d, ids, counts):
    """the same lists through every entry point: {name: (idx, dist, cnt)}"""
    import torch

    from lab_1806_vec_db_amd.shard import ShardExchange

    got = {}
    plain = [_dev(d), _dev(ids), _dev(counts)]
    ex = ShardExchange(nq, k, "cuda", S)
    buf = torch.from_numpy(M.pack_blocks(ex, d, ids, counts)).cuda()
    layout = (buf.data_ptr(), ex.block, ex.off_ids, ex.off_dists, ex.off_counts, S, nq, k)
    torch.cuda.synchronize()
    o = _outs(nq, k)
    ix.merge_topk_device(*_ptrs(plain), S, nq, k, *_ptrs(o))
    got["device"] = _read(o)
    o = _outs(nq, k)
    ix.merge_topk_gathered(*layout, *_ptrs(o))
    got["gathered"] = _read(o)
    if k <= 64:
        o = _outs(nq, k)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ix.merge_topk_gathered_async(*layout, *_ptrs(o), stream=side.cuda_stream)
        side.synchronize()
        got["async"] = _read(o)
    return got


@pytest.mark.parametrize("nq", M.NQS)
@pytest.mark.parametrize("S,k", M.SHAPES_K64 + M.SHAPES_LISTS)
def test_constructed_lists_through_every_entry_point(ix, S, k, nq):
    (d, ids, counts), exp = _case(S, k, nq)
    got = _merge_three_ways(ix, S, k, nq, d, ids, counts)
    assert len(got) == (3 if k <= 64 else 2)
    for name, g in got.items():
        M.same(g, exp, (name, S, k, nq))


def test_largest_input_64_lists_of_1024(ix):
    S, k = M.SHAPE_LARGEST
    (d, ids, counts), exp = _case(S, k, 2)
    for name, g in _merge_three_ways(ix, S, k, 2, d, ids, counts).items():
        M.same(g, exp, (name, S, k))


def test_odd_block_has_a_poisoned_pad(ix):
    """nq*k odd: the block layout leaves four bytes between the distances and the counts, 0xFF here"""
    from lab_1806_vec_db_amd.shard import ShardExchange

    S, k, nq = 4, 3, 5
    ex = ShardExchange(nq, k, "cpu", S)
    assert ex.off_counts - (ex.off_dists + nq * k * 4) == 4
    (d, ids, counts), exp = _case(S, k, nq)
    got = _merge_three_ways(ix, S, k, nq, d, ids, counts)
    assert set(got) == {"device", "gathered", "async"}
    for name, g in got.items():
        M.same(g, exp, name)


def test_refused_calls_raise_and_leave_the_process_usable(ix):
    import torch

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.shard import ShardExchange

    S, k, nq = 3, 10, 5
    (d, ids, counts), exp = _case(S, k, nq)
    plain = [_dev(d), _dev(ids), _dev(counts)]
    ex = ShardExchange(nq, k, "cuda", S)
    buf = torch.from_numpy(M.pack_blocks(ex, d, ids, counts)).cuda()
    big = _outs(nq, 1025)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def layout(n_shards, kk):
        return (buf.data_ptr(), ex.block, ex.off_ids, ex.off_dists, ex.off_counts, n_shards, nq, kk)

    for n_shards, kk, what in ((S, 0, "k must be"), (S, 1025, "k must be"), (0, k, "at least one shard")):
        with pytest.raises(vdb.VdbError, match=what):
            ix.merge_topk_device(*_ptrs(plain), n_shards, nq, kk, *_ptrs(big))
        with pytest.raises(vdb.VdbError, match=what):
            ix.merge_topk_gathered(*layout(n_shards, kk), *_ptrs(big))
    for n_shards, kk, what in ((S, 0, "k in 1..64"), (S, 65, "k in 1..64"), (0, k, "at least one shard")):
        with pytest.raises(vdb.VdbError, match=what):
            ix.merge_topk_gathered_async(*layout(n_shards, kk), *_ptrs(big), stream=side.cuda_stream)
    side.synchronize()
    assert all((t.view(torch.uint8) == SENTINEL).all().item() for t in big)  # a refused call writes nothing
    for name, g in _merge_three_ways(ix, S, k, nq, d, ids, counts).items():
        M.same(g, exp, ("after the refusals", name))


def _search_shards(shards, qs, k):
    """flat_knn_device of every shard into [S][nq][k] tensors (pre-filled with poison: -inf under unused ids)"""
    import torch

    S, nq = len(shards), len(qs)
    d_q = torch.from_numpy(qs).cuda()
    t_idx = torch.full((S, nq, k), (1 << 31) + 12345, dtype=torch.int64, device="cuda")
    t_dist = torch.full((S, nq, k), float("-inf"), dtype=torch.float32, device="cuda")
    t_cnt = torch.zeros((S, nq), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for s, sx in enumerate(shards):
        sx.flat_knn_device(d_q.data_ptr(), nq, k, t_idx[s].data_ptr(), t_dist[s].data_ptr(), t_cnt[s].data_ptr())
    return t_dist, t_idx, t_cnt


def test_ids_up_to_2_pow_32_merge_and_one_more_is_refused():
    """a 10-row shard at id offset 2^32 - 10 holds the ids up to 2^32 - 1: all three device merges carry them.  One row further the
    last id needs 33 bits, which a pair key does not have: the merges refuse the shard instead of truncating the id."""
    import torch

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.shard import ShardExchange
    from oracle import oracle as O

    rng = np.random.default_rng(7)
    base = rng.standard_normal((20, 8)).astype(np.float32)
    base[15] = base[3]  # a tie across the two shards
    qs = np.concatenate([base[3:4], rng.standard_normal((4, 8)).astype(np.float32)])
    nq, k, off = len(qs), 12, (1 << 32) - 10
    lo, hi = vdb.GpuIndex(8, "l2sqr"), vdb.GpuIndex(8, "l2sqr")
    try:
        lo.batch_add(base[:10])
        hi.batch_add(base[10:])
        hi.set_id_offset(off)
        t_dist, t_idx, t_cnt = _search_shards([lo, hi], qs, k)
        assert t_cnt.cpu().tolist() == [[10] * nq] * 2
        oi, od, _ = O.flat_knn_batch(base, qs, k, 0)
        oi = oi.astype(np.uint64)
        exp = (np.where(oi >= 10, oi + np.uint64(off - 10), oi), od, np.full(nq, k, dtype=np.uint64))
        assert int(exp[0].max()) == M.ID_TOP and exp[0][0, :2].tolist() == [3, off + 5]
        d, ids, counts = t_dist.cpu().numpy(), t_idx.cpu().numpy().view(np.uint64), t_cnt.cpu().numpy().view(np.uint64)
        M.same(M.merge_topk_ref(d, ids, counts, k), exp, "reference merge vs oracle")
        for name, g in _merge_three_ways(hi, 2, k, nq, d, ids, counts).items():
            M.same(g, exp, name)
        hi.set_id_offset(off + 1)
        ex = ShardExchange(nq, k, "cuda", 2)
        buf = torch.from_numpy(M.pack_blocks(ex, d, ids, counts)).cuda()
        layout = (buf.data_ptr(), ex.block, ex.off_ids, ex.off_dists, ex.off_counts, 2, nq, k)
        o = _outs(nq, k)
        torch.cuda.synchronize()
        with pytest.raises(vdb.VdbError, match="fit 32 bits"):
            hi.merge_topk_device(t_dist.data_ptr(), t_idx.data_ptr(), t_cnt.data_ptr(), 2, nq, k, *_ptrs(o))
        with pytest.raises(vdb.VdbError, match="fit 32 bits"):
            hi.merge_topk_gathered(*layout, *_ptrs(o))
        with pytest.raises(vdb.VdbError, match="fit 32 bits"):
            hi.merge_topk_gathered_async(*layout, *_ptrs(o), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert all((t.view(torch.uint8) == SENTINEL).all().item() for t in o)
    finally:
        lo.close()
        hi.close()
