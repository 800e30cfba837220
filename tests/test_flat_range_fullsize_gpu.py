"""GPU: exact Flat range search at BASELINE.json's full size (1,000,000 x 960 f32, 256 queries: the fixture shape of
test_fullsize_gpu.py).  The CPU oracle needs ~1 s per query per core here, so most of the check is against the library's own exact
k-NN (itself checked against the oracle at this size) and the strict-order scan; 16 queries go to the oracle itself.

Radii: r_q = the query's 10th exact distance (result == that top-10, plus ties), and 1.03 x that distance (a few hundred results
per query on this generator).  At the first radius at least 7/8 of the queries must be answered by the 8-bit tier -- the project's
own 1/8 rule for a tier that earns its place -- otherwise the test would pass on the scan alone and show nothing about the new path.
At the second the tier's share and hits / results are printed (recorded), not gated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, K = 1_000_000, 960, 10
STATS = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits", "flat_range_results")


@pytest.fixture(scope="module")
def world():
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    base = gist_like_gpu(torch, N, DIM, 1806, dev)
    qs = gist_like_gpu(torch, 256, DIM, 1807, dev).cpu().numpy()
    yield vdb, torch, base, qs
    del base
    torch.cuda.empty_cache()


def _stats(ix):
    return {s: ix.get_stat(s) for s in STATS}


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(a[1], b[1]), what
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), what


def _run(world, dist, kind):
    vdb, torch, base, qs = world
    from oracle import oracle as O

    ix = vdb.GpuIndex(DIM, dist)
    try:
        ix.add_device(base.data_ptr(), N)
        ki, kd, kc = ix.flat_knn(qs, 64)
        assert (kc == 64).all()
        r10 = kd[:, K - 1].copy()
        # ---- r = the 10th distance: the top-10 plus ties
        s0 = _stats(ix)
        lims, idx, dist_ = got = ix.range_search(qs, r10)
        d = {s: _stats(ix)[s] - s0[s] for s in STATS}
        print(dist, "r = d10:", d)
        for q in range(len(qs)):
            a, b = int(lims[q]), int(lims[q + 1])
            ties = int((kd[q] <= r10[q]).sum())
            assert 10 <= ties < 64 and b - a == ties, (q, a, b, ties)
            assert np.array_equal(idx[a:b], ki[q, :ties]) and np.array_equal(dist_[a:b].view(np.uint32), kd[q, :ties].view(np.uint32)), q
        assert d["flat_range_queries"] == len(qs) and d["flat_range_results"] == int(lims[-1])
        assert d["flat_range_i8_queries"] * 8 >= 7 * len(qs), d  # the tier answers at least 7/8 of the queries
        ix.set_flat_mode(1)
        scan = ix.range_search(qs[:24], r10[:24])
        ix.set_flat_mode(0)
        sub = (lims[:25], idx[:int(lims[24])], dist_[:int(lims[24])])
        _same(sub, scan, "mode 0 == mode 1, r = d10")
        # ... and the oracle itself on 16 queries
        host = base.cpu().numpy()
        oi, od, oc = O.flat_knn_batch(host, qs[:16], 64, kind, nthreads=16)
        del host
        for q in range(16):
            a, b = int(lims[q]), int(lims[q + 1])
            cut = int((od[q] <= r10[q]).sum())
            assert cut < 64 and b - a == cut
            assert np.array_equal(idx[a:b], oi[q, :cut].astype(np.uint64)) and np.array_equal(dist_[a:b].view(np.uint32), od[q, :cut].view(np.uint32))
        # ---- r = 1.03 x the 10th distance: a few hundred results per query; equality with the scan on 24 queries is required, the
        # tier's share and hits / results are recorded
        r103 = (r10 * np.float32(1.03)).astype(np.float32)
        s0 = _stats(ix)
        got = ix.range_search(qs, r103)
        d = {s: _stats(ix)[s] - s0[s] for s in STATS}
        per_q = np.diff(got[0].astype(np.int64))
        print(dist, "r = 1.03 d10:", d, "results per query min / mean / max:", int(per_q.min()), float(per_q.mean()), int(per_q.max()),
              "hits / results:", d["flat_range_hits"] / max(1, d["flat_range_results"]))
        ix.set_flat_mode(1)
        scan = ix.range_search(qs[:24], r103[:24])
        ix.set_flat_mode(0)
        e = int(got[0][24])
        _same((got[0][:25], got[1][:e], got[2][:e]), scan, "mode 0 == mode 1, r = 1.03 d10")
        for q in range(len(qs)):  # ascending by (distance, index), everything inside the radius, the top-64 reproduced
            a, b = int(got[0][q]), int(got[0][q + 1])
            pairs = list(zip(got[2][a:b].tolist(), got[1][a:b].tolist()))
            assert pairs == sorted(pairs) and (got[2][a:b] <= r103[q]).all()
            m = min(b - a, 64)
            assert np.array_equal(got[1][a:a + m], ki[q, :m])
        # self-queries at r = 0 (L2Sqr: the row itself at distance exactly 0)
        rows = [0, 12345, N - 1]
        sq = base[rows].cpu().numpy()
        sl, si, sd = ix.range_search(sq, 0.0 if kind == 0 else 1e-6)
        for j, r in enumerate(rows):
            assert r in si[int(sl[j]):int(sl[j + 1])].tolist()
            if kind == 0:
                assert (sd[int(sl[j]):int(sl[j + 1])] == 0.0).all()
        # the k-NN tier's counters were moved by the k-NN call alone
        assert ix.get_stat("flat_i8_queries") == len(qs)
    finally:
        ix.close()
        torch.cuda.empty_cache()


def test_range_full_size_l2sqr(world):
    _run(world, "l2sqr", 0)


def test_range_full_size_cosine(world):
    _run(world, "cosine", 1)
