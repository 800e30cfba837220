"""GPU: many row shards on one GPU, end to end, and the exchange code of shard.py above the device merges.

One GPU stands in for S (as in test_range_merge_gpu.py): a gist-like 6 000 x 64 table is split into S GpuIndex objects with
set_id_offset, every shard's flat_knn_device result lands in [S][nq][k] tensors and merge_topk_device merges them; the expected answer
is the oracle's UNSHARDED flat_knn on the whole table, bit for bit.

The exchange (allgather_merge, allgather_merge_pq, ShardExchange.exchange_merge with world > 1) needs a collective.  Here one
process plays the S ranks against a stand-in: three functions of torch.distributed are patched in the test, and every rank's call
runs twice -- first against a collective that only records what the rank sends (and ends the call there), then against one that
delivers the S recorded buffers.  Every "rank" must end with the unsharded oracle answer.

The recording collective does more than record: it raises _Recorded, so the first pass of a rank ends at the collective and nothing
merges a receive buffer that nobody filled.  Each rank's merge (the enqueued one of ShardExchange included) therefore runs once, in the
second pass, not twice."""
import numpy as np
import pytest

from conftest import gist_like

import merge_ref as M

pytestmark = pytest.mark.gpu

DISTS = (("l2sqr", 0), ("cosine", 1))
N, DIM, KMAX = 6000, 64, 1024
KS = (1, 10, 64, 65, 200, 1024)
UNEVEN = [(0, 40), (40, 40), (40, 3000), (3000, N)]  # fewer rows than k, no rows


@pytest.fixture(scope="module")
def table():
    from oracle import oracle as O

    base = gist_like(N, dim=DIM, seed=1806)
    base[5000:5005] = base[10:15]  # duplicated rows on different shards of every split ...
    base[2990:2993] = base[3010:3013]
    qs = gist_like(12, dim=DIM, seed=1807)
    qs[:5] = base[10:15]  # ... and queries on them: distance ties across shards at the head of the list
    qs[5:8] = base[3010:3013]
    full = {}
    for _, kind in DISTS:
        oi, od, oc = O.flat_knn_batch(base, qs, KMAX, kind, nthreads=16)
        assert (oc == KMAX).all()
        full[kind] = (oi.astype(np.uint64), od)
    return base, qs, full


def _expect(full, k):
    oi, od = full
    return oi[:, :k], np.ascontiguousarray(od[:, :k]), np.full(len(oi), k, dtype=np.uint64)


def _shards(dist, base, bounds):
    import lab_1806_vec_db_amd as vdb

    out = []
    for r0, r1 in bounds:
        sx = vdb.GpuIndex(base.shape[1], dist)
        if r1 > r0:
            sx.batch_add(base[r0:r1])
        sx.set_id_offset(r0)
        out.append(sx)
    return out


def _search(sx, d_q, nq, k, t_idx, t_dist, t_cnt):
    sx.flat_knn_device(d_q.data_ptr(), nq, k, t_idx.data_ptr(), t_dist.data_ptr(), t_cnt.data_ptr())


def _poisoned(shape_prefix, k):
    """result tensors of a search, pre-filled: whatever a shard does not write is -inf under an id no row has"""
    import torch

    return (torch.full(shape_prefix + (k,), (1 << 31) + 4242, dtype=torch.int64, device="cuda"),
            torch.full(shape_prefix + (k,), float("-inf"), dtype=torch.float32, device="cuda"),
            torch.zeros(shape_prefix, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("split", [2, 3, 8, "uneven"])
@pytest.mark.parametrize("dist,kind", DISTS)
def test_shards_searched_and_merged_on_the_device_equal_the_unsharded_oracle(table, dist, kind, split):
    import torch

    from lab_1806_vec_db_amd.shard import shard_bounds

    base, qs, full = table
    bounds = UNEVEN if split == "uneven" else [shard_bounds(N, split, r) for r in range(split)]
    shards = _shards(dist, base, bounds)
    S, nq = len(shards), len(qs)
    try:
        d_q = torch.from_numpy(qs).cuda()
        for k in KS:
            t_idx, t_dist, t_cnt = _poisoned((S, nq), k)
            torch.cuda.synchronize()
            for s, sx in enumerate(shards):
                _search(sx, d_q, nq, k, t_idx[s], t_dist[s], t_cnt[s])
            assert t_cnt.cpu().tolist() == [[min(k, r1 - r0)] * nq for r0, r1 in bounds]
            o_idx, o_dist, o_cnt = _poisoned((nq,), k)
            torch.cuda.synchronize()
            shards[-1].merge_topk_device(t_dist.data_ptr(), t_idx.data_ptr(), t_cnt.data_ptr(), S, nq, k, o_idx.data_ptr(),
                                         o_dist.data_ptr(), o_cnt.data_ptr())
            M.same((o_idx.cpu().numpy(), o_dist.cpu().numpy(), o_cnt.cpu().numpy()), _expect(full[kind], k), (dist, split, k))
    finally:
        for sx in shards:
            sx.close()


class _Recorded(Exception):
    """the recording collective ends a rank's first pass here: nothing downstream runs on a buffer nobody filled"""


class _StandInCollective:
    """all_gather_into_tensor for one process that plays S ranks: pass 1 records the tensor the rank sends, pass 2 delivers the
    S recorded tensors in rank order"""

    def __init__(self, world):
        self.world, self.sent, self.deliver, self.rank = world, [], False, None

    def install(self, monkeypatch):
        import torch.distributed as dist

        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: self.world)
        monkeypatch.setattr(dist, "all_gather_into_tensor", self)

    def __call__(self, out, inp, group=None):
        import torch

        if not self.deliver:
            assert len(self.sent) == self.rank
            self.sent.append(inp.detach().clone())
            raise _Recorded
        assert len(self.sent) == self.world and torch.equal(inp, self.sent[self.rank])
        assert out.numel() == self.world * inp.numel() and out.dtype == inp.dtype and out.is_contiguous()
        out.view(-1).copy_(torch.cat([t.reshape(-1) for t in self.sent]))

    def run(self, call):
        """call(rank) on every rank, twice; the results of the second pass"""
        self.sent, self.deliver = [], False
        for r in range(self.world):
            self.rank = r
            with pytest.raises(_Recorded):
                call(r)
        self.deliver = True
        out = []
        for r in range(self.world):
            self.rank = r
            out.append(call(r))
        return out


def _np(result):
    import torch

    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in result)


@pytest.mark.parametrize("k", [10, 100])
def test_allgather_merge_on_cuda_tensors(table, monkeypatch, k):
    import torch

    from lab_1806_vec_db_amd.shard import allgather_merge, shard_bounds

    base, qs, full = table
    S, nq = 3, len(qs)
    shards = _shards("l2sqr", base, [shard_bounds(N, S, r) for r in range(S)])
    try:
        d_q = torch.from_numpy(qs).cuda()
        local = []
        for sx in shards:
            t = _poisoned((nq,), k)
            torch.cuda.synchronize()
            _search(sx, d_q, nq, k, *t)
            local.append(t)
        coll = _StandInCollective(S)
        coll.install(monkeypatch)
        results = coll.run(lambda r: allgather_merge(*local[r], k, gpu_index=shards[r]))
        for r, res in enumerate(results):
            M.same(_np(res), _expect(full[0], k), ("rank", r, k))
    finally:
        for sx in shards:
            sx.close()


@pytest.mark.parametrize("k", [10, 100])
def test_shard_exchange_with_a_world_of_three(table, monkeypatch, k):
    """k = 10: the enqueued merge (merge_topk_gathered_async on torch's stream); k = 100: the synchronous scratch-list merge"""
    import torch

    from lab_1806_vec_db_amd.shard import ShardExchange, shard_bounds

    base, qs, full = table
    S, nq = 3, len(qs)
    shards = _shards("l2sqr", base, [shard_bounds(N, S, r) for r in range(S)])
    try:
        d_q = torch.from_numpy(qs).cuda()
        exs = [ShardExchange(nq, k, "cuda", world=S) for _ in range(S)]  # (every rank owns its exchange)
        for sx, ex in zip(shards, exs):
            assert ex.active and ex.depth == 2
            idx, dist, cnt = ex.begin_step()
            torch.cuda.synchronize()
            _search(sx, d_q, nq, k, idx, dist, cnt)
        coll = _StandInCollective(S)
        coll.install(monkeypatch)

        def rank_step(r):
            res = exs[r].exchange_merge(shards[r])
            exs[r].wait()
            return tuple(t.clone() for t in res)

        for r, res in enumerate(coll.run(rank_step)):
            M.same(_np(res), _expect(full[0], k), ("rank", r, k))
    finally:
        for sx in shards:
            sx.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_allgather_merge_pq_on_cuda_tensors(table, monkeypatch, dist, kind):
    import torch

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.shard import allgather_merge_pq, shard_bounds
    from oracle import oracle as O

    base, qs, _ = table
    S, nq = 3, len(qs)
    whole = vdb.GpuIndex(DIM, dist)
    whole.batch_add(base)
    whole.pq_build(n_bits=4, m=16, train_n=2000, max_iter=4, seed=5)
    cent = whole.pq_export()["centroids"]
    whole.close()
    opq = O.PQ.from_centroids(DIM, 16, 4, kind, cent)
    opq.encode_all(base)
    shards = _shards(dist, base, [shard_bounds(N, S, r) for r in range(S)])
    try:
        for sx in shards:
            sx.pq_attach(4, 16, cent, None)  # centroids replicated, codes encoded per shard
        d_q = torch.from_numpy(qs).cuda()
        for k, ef in ((10, 100), (100, 100), (5, 1500)):
            efk = max(k, ef)
            keys = []
            for sx in shards:
                adc = torch.zeros((nq, efk), dtype=torch.int64, device="cuda")
                ex = torch.zeros((nq, efk), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                sx.knn_pq_shard_device(d_q.data_ptr(), nq, k, ef, adc.data_ptr(), ex.data_ptr())
                keys.append((adc, ex))
            coll = _StandInCollective(S)
            coll.install(monkeypatch)
            results = coll.run(lambda r: allgather_merge_pq(*keys[r], k, gpu_index=shards[r]))
            exp_i = np.zeros((nq, k), dtype=np.uint64)
            exp_d = np.zeros((nq, k), dtype=np.float32)
            for q in range(nq):
                oi, od = O.flat_knn_pq(base, opq, qs[q], k, ef, kind)
                assert len(oi) == k
                exp_i[q], exp_d[q] = oi, od
            for r, res in enumerate(results):
                M.same(_np(res), (exp_i, exp_d, np.full(nq, k, dtype=np.uint64)), (dist, "rank", r, k, ef))
    finally:
        for sx in shards:
            sx.close()
