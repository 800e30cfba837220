"""GPU: GpuIndex.flat_knn_vote end to end on 2000 x 32 rows, both metrics: the vote against vote_ref (test_vote_lists_gpu.py) applied to
what flat_knn / flat_knn_filtered_multi return at the same k, bit for bit."""
import numpy as np
import pytest

from test_vote_lists_gpu import NONE, vote_ref

pytestmark = pytest.mark.gpu

N, DIM, NQ = 2000, 32, 9
C_TEN, C_SKEW = 0, 3


@pytest.fixture(scope="module", params=["l2sqr", "cosine"])
def env(request):
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, DIM)).astype(np.float32)
    x[100:120] = x[100]  # equal rows: equal distances, ordered by id
    cols = {C_TEN: (rng.integers(0, 10, N)).astype(np.uint32),
            C_SKEW: rng.choice(np.array([1, 2, 3, 0xFFFFFFFE, NONE], dtype=np.uint32), size=N, p=[0.7, 0.1, 0.05, 0.05, 0.1])}
    ixs = {}
    for scalar in ("f32", "u8"):
        ix = vdb.GpuIndex(DIM, request.param, device=0, scalar=scalar)
        if scalar == "f32":
            ix.batch_add(x)
        else:
            ix.batch_add_u8(np.clip(x * 40 + 128, 0, 255).astype(np.uint8))
        for c, v in cols.items():
            ix.set_labels(c, v)
        ixs[scalar] = ix
    q = np.concatenate([x[100:101], rng.standard_normal((NQ - 1, DIM)).astype(np.float32)])
    yield ixs, cols, q, rng
    for ix in ixs.values():
        ix.close()


def _expect(col, lists, c, mode, eps):
    idx, dist, cnt = lists
    return [vote_ref(col[idx[j, :int(cnt[j])].astype(np.int64)], dist[j, :int(cnt[j])], c, mode, eps) for j in range(idx.shape[0])]


def _same(got, want):
    for j, (code, score, votes, n, voters) in enumerate(want):
        assert got[0][j].tolist() == code.tolist() and got[2][j].tolist() == votes.tolist(), j
        assert got[1][j].view(np.uint32).tolist() == score.view(np.uint32).tolist(), j
        assert (int(got[3][j]), int(got[4][j])) == (n, voters), j


@pytest.mark.parametrize("mode", ["uniform", "inverse"])
@pytest.mark.parametrize("column,k,c", [(C_TEN, 10, 1), (C_TEN, 40, 10), (C_SKEW, 128, 3), (C_SKEW, 1100, 5)])
def test_unfiltered(env, column, k, c, mode):
    ixs, cols, q, _ = env
    ix = ixs["f32"]
    before = ix.get_stat("flat_vote_queries"), ix.get_stat("flat_vote_scratch")
    _same(ix.flat_knn_vote(q, k, column, c, mode, 1e-3), _expect(cols[column], ix.flat_knn(q, k), c, mode, 1e-3))
    assert ix.get_stat("flat_vote_queries") - before[0] == NQ
    assert ix.get_stat("flat_vote_scratch") - before[1] == (NQ if k > 1024 else 0)


@pytest.mark.parametrize("mode", ["uniform", "inverse"])
def test_masks(env, mode):
    ixs, cols, q, rng = env
    ix = ixs["f32"]
    masks = [ix.make_mask(rng.random(N) < 0.5), ix.make_mask(np.arange(0, 30)), ix.make_mask(cols[C_TEN] == 4)]
    try:
        for mask_of in (np.zeros(NQ, np.uint32), (np.arange(NQ) % 3).astype(np.uint32)):  # one mask | one per query; mask 1 has m = 30 < k
            lists = ix.flat_knn_filtered_multi(q, 40, masks, mask_of)
            for column in (C_TEN, C_SKEW):
                _same(ix.flat_knn_vote(q, 40, column, 4, mode, 1e-6, masks, mask_of), _expect(cols[column], lists, 4, mode, 1e-6))
        # one RowMask for every query, and c past its 30 rows
        _same(ix.flat_knn_vote(q, 40, C_SKEW, 35, mode, 1e-6, masks[1]), _expect(cols[C_SKEW], ix.flat_knn_filtered_multi(q, 40, masks[1:2], np.zeros(NQ)), 35, mode, 1e-6))
    finally:
        for m in masks:
            m.close()


def test_u8_index_and_device_form(env):
    import torch

    ixs, cols, q, _ = env
    ix = ixs["u8"]
    _same(ix.flat_knn_vote(q, 64, C_SKEW, 3, "inverse", 0.5), _expect(cols[C_SKEW], ix.flat_knn(q, 64), 3, "inverse", 0.5))
    m = ix.make_mask(np.arange(50))
    try:
        import lab_1806_vec_db_amd as vdb

        with pytest.raises(vdb.VdbError, match="f32 rows"):
            ix.flat_knn_vote(q, 64, C_SKEW, 3, masks=m)
    finally:
        m.close()
    ix = ixs["f32"]
    t_q = torch.from_numpy(q).cuda()
    outs = [torch.zeros((NQ, 3), dtype=torch.int32, device="cuda"), torch.zeros((NQ, 3), dtype=torch.float32, device="cuda"),
            torch.zeros((NQ, 3), dtype=torch.int32, device="cuda"), torch.zeros(NQ, dtype=torch.int64, device="cuda"),
            torch.zeros(NQ, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    ix.flat_knn_vote_device(t_q.data_ptr(), NQ, 40, C_TEN, 3, *[t.data_ptr() for t in outs], mode="inverse", eps=1e-3)
    host = ix.flat_knn_vote(q, 40, C_TEN, 3, "inverse", 1e-3)
    for t, h in zip(outs, host):
        assert t.cpu().numpy().tobytes() == h.tobytes()
    _same(host, _expect(cols[C_TEN], ix.flat_knn(q, 40), 3, "inverse", 1e-3))
