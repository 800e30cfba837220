"""GPU: exact Flat range search on the 4 500 000 x 960 index of test_large_rows_gpu.py (n * d > 2^32: every row offset of the
hit evaluation, the scan and the result assembly must be formed in 64 bits).  Same fixture, same construction: the planted rows
are far closer to the queries than any bulk row, so a query's 10th distance as radius returns exactly its known top-10."""
import numpy as np
import pytest

from test_large_rows_gpu import ANCHORS, DIM, K, N, QPA, world  # noqa: F401  (the module-scoped fixture is rebuilt for this module)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dist,kind", [("l2sqr", 0), ("cosine", 1)])
def test_range_past_4gib(world, dist, kind):  # noqa: F811
    import lab_1806_vec_db_amd as vdb

    torch, base, anchors, qs, pos, special, expect = world
    ei, ed = expect[kind]
    sel = slice(None, None, QPA)  # 16 queries, one per anchor
    q16, r16 = qs[sel], ed[sel, K - 1].copy()
    ix = vdb.GpuIndex(DIM, dist)
    try:
        ix.add_device(base.data_ptr(), N)
        ix.set_flat_mode(2)
        lims, idx, d = tier = ix.range_search(q16, r16)
        assert ix.get_stat("flat_range_i8_queries") == ANCHORS and ix.get_stat("flat_range_scan_queries") == 0
        ix.set_flat_mode(1)
        scan = ix.range_search(q16, r16)
        assert ix.get_stat("flat_range_scan_queries") == ANCHORS
        for a, b in zip(tier, scan):
            assert np.array_equal(a, b)
        assert np.array_equal(d.view(np.uint32), scan[2].view(np.uint32))
        for q in range(ANCHORS):
            a, b = int(lims[q]), int(lims[q + 1])
            assert b - a >= K and (d[a:b] <= r16[q]).all()  # (more than K only by ties at the 10th distance)
            assert np.array_equal(idx[a:a + K], ei[sel][q]) and np.array_equal(d[a:a + K].view(np.uint32), ed[sel][q].view(np.uint32))
        assert (idx > np.uint64(2**32 // DIM)).any()  # rows past the 2^32-element offset are among the answers
        # the last rows of the table as self-queries at r = 0
        last = [N - 1, N - 2]
        sq = base[last].cpu().numpy()
        for mode in (2, 1):
            ix.set_flat_mode(mode)
            sl, si, sd = ix.range_search(sq, 0.0 if kind == 0 else 1e-6)
            for j, r in enumerate(last):
                got = si[int(sl[j]):int(sl[j + 1])].tolist()
                assert r in got and len(got) < 8, (mode, got)
                if kind == 0:
                    assert got == [r] and sd[int(sl[j])] == 0.0
    finally:
        ix.close()
        torch.cuda.empty_cache()
