"""GPU: the two unit epilogues of the 8-bit filter kernel (k_flat_gemm8, parameter "flat_gemm8_epi").

0 (default): keys from scalar f32 multiply / fma, the wave's stage of passed lanes carried over units and drained when the next
(tile, half) pair would not fit and before every hand-over of the workgroup's hit buffer.  1: the earlier form (packed f32 arithmetic,
one drain per unit).  A key is one rounded multiply and one fused fma either way, so the two forms must give the SAME BITS: dense
keys, thresholds, hit lists and answers -- and the answers must be the oracle's.  The switch is process-wide: every test puts it
back to 0.
"""
import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

FORMS = (0, 1)


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


def _check_all(idx, d, cnt, oi, od, oc):
    assert cnt.tolist() == oc.tolist()
    for q in range(idx.shape[0]):
        assert idx[q].tolist() == oi[q].tolist(), (q, idx[q], oi[q])
        assert np.array_equal(d[q], od[q]), (q, d[q], od[q])


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _both_forms(ix, qs, k):
    """one search per epilogue form with the hits-per-query counter beside it: ((idx, d, cnt), hits) for form 0 and form 1"""
    out = []
    for epi in FORMS:
        ix.set_param("flat_gemm8_epi", epi)
        ix.set_param("flat_i8_stats", 1)  # (resets the counters)
        r = ix.flat_knn(qs, k)
        out.append((r, ix.get_stat("flat_i8_hits_sum"), ix.get_stat("flat_i8_hits_max")))
    ix.set_param("flat_gemm8_epi", 0)
    _same(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:], (out[0][1:], out[1][1:])  # the same hits per query: nothing lost in a carried stage, nothing twice
    return out[0][0]


def _reset(ix):
    for name in ("flat_gemm8_epi", "flat_gemm8_res", "flat_gemm8_kc", "flat_gemm8_burst", "flat_gemm8_nt", "flat_gemm8_coop"):
        ix.set_param(name, 0)


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
@pytest.mark.parametrize("name,dim,n", [("gist", 960, 6011), ("normal", 128, 6000), ("decades", 320, 5990)])
def test_dense_keys_are_bit_identical(mods, name, dim, n, dist):
    """the sample path: the dense keys of every (row, query) pair, resident and chunked kernel forms, ragged last unit"""
    vdb, _ = mods
    rng = np.random.default_rng(dim + n)
    if name == "gist":
        base, qs = gist_like(n, dim=dim, seed=3), gist_like(140, dim=dim, seed=4)
    else:
        base = rng.standard_normal((n, dim)).astype(np.float32)
        if name == "decades":
            base *= np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(n, 1))).astype(np.float32)
        qs = rng.standard_normal((140, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, dist)
    ix.batch_add(base)
    try:
        for res in (0, 1):
            ix.set_param("flat_gemm8_res", res)
            keys = []
            for epi in FORMS:
                ix.set_param("flat_gemm8_epi", epi)
                k, _, _, _ = ix.flat_shortlist_keys(qs, 2)
                keys.append(k.view(np.uint32).copy())
            assert keys[0].shape == (140, n) and np.array_equal(keys[0], keys[1]), (name, dim, res, int((keys[0] != keys[1]).sum()))
    finally:
        _reset(ix)
        ix.close()


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_unit_minima_sample_gives_the_same_thresholds(mods, dist):
    """the sample path with one value per (query, sampled unit) forced (flat_i8_unit_min = 2) and with the dense sample (1): the thresholds
    decide the hits per query, which must not depend on the epilogue form, and the answers are the oracle's"""
    vdb, O = mods
    n, dim, nq = 130011, 128, 300
    rng = np.random.default_rng(21)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, dist)
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        res = []
        for um in (2, 1):
            ix.set_param("flat_i8_unit_min", um)
            res.append(_both_forms(ix, qs, 10))
        _same(res[0], res[1])
        sel = np.arange(0, nq, 6)
        oi, od, oc = O.flat_knn_batch(base, qs[sel], 10, O.L2SQR if dist == "l2sqr" else O.COSINE, nthreads=8)
        _check_all(res[0][0][sel], res[0][1][sel], res[0][2][sel], oi, od, oc)
    finally:
        _reset(ix)
        ix.close()


@pytest.mark.parametrize("dim,n,nq", [(960, 40000, 200), (128, 50000, 130), (320, 20000, 70)])
def test_every_kernel_form(mods, dim, n, nq):
    """every kernel form tests/test_flat_i8_gpu.py::test_i8_pass_parity cycles through -- resident with rings of 5 / 3 / 2, chunked with every
    staging form, non-temporal loads -- under both epilogues: identical to each other and to the oracle"""
    vdb, O = mods
    if dim == 960:
        base, qs = gist_like(n, seed=41), gist_like(nq, seed=42)
    else:
        rng = np.random.default_rng(dim + 7)
        base = rng.standard_normal((n, dim)).astype(np.float32)
        qs = rng.standard_normal((nq, dim)).astype(np.float32)
    base[n - 1] = base[0]
    oi, od, oc = O.flat_knn_batch(base, qs, 10, 0, nthreads=8)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        for res, kc, burst in ((0, 0, 0), (0, 5, 0), (0, 3, 0), (0, 2, 0), (1, 5, 0), (1, 3, 1), (1, 3, 2), (1, 2, 1), (1, 2, 2), (1, 0, 0)):
            ix.set_param("flat_gemm8_res", res)
            ix.set_param("flat_gemm8_kc", kc)
            ix.set_param("flat_gemm8_burst", burst)
            idx, d, cnt = _both_forms(ix, qs, 10)
            _check_all(idx, d, cnt, oi, od, oc)
        _reset(ix)
        for nt in (1, 2):
            ix.set_param("flat_gemm8_nt", nt)
            idx, d, cnt = _both_forms(ix, qs, 10)
            _check_all(idx, d, cnt, oi, od, oc)
        assert ix.get_stat("flat_i8_queries") == 2 * 12 * nq  # the 8-bit pass took every one of these calls
    finally:
        _reset(ix)
        ix.close()


@pytest.mark.parametrize("dim,n,nq", [(128, 130000, 1024), (960, 100000, 512), (192, 99000, 256 + 128)])
def test_cooperative_sets_and_three_groups(mods, dim, n, nq):
    """cooperative sets of 8 and of 4 (the hit buffer handed over in blocks of units: the stage is drained before each) and a 3-group call
    without sets, with the sets switched off as well"""
    vdb, O = mods
    rng = np.random.default_rng(n + nq)
    if dim == 960:
        base, qs = gist_like(n, seed=77), gist_like(nq, seed=78)
    else:
        base = rng.standard_normal((n, dim)).astype(np.float32)
        qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        a = _both_forms(ix, qs, 10)
        groups = (nq + 127) // 128
        assert ix.get_stat("flat_gemm8_coop_sets") == (8 if groups % 8 == 0 else 4 if groups % 4 == 0 else 0)
        ix.set_param("flat_gemm8_coop", 1)
        b = _both_forms(ix, qs, 10)
        assert ix.get_stat("flat_gemm8_coop_sets") <= 1
        _same(a, b)
        sel = rng.choice(nq, 48, replace=False)
        oi, od, oc = O.flat_knn_batch(base, qs[sel], 10, 0, nthreads=8)
        _check_all(a[0][sel], a[1][sel], a[2][sel], oi, od, oc)
    finally:
        _reset(ix)
        ix.close()


def test_stage_carried_over_unit_boundaries(mods):
    """hits that cluster in a few units: 400 consecutive rows lie next to every query, so in their units all 64 lanes of most (tile, half)
    pairs pass -- the stage fills in mid-unit, is drained there, and what is left is carried into the next unit; the rows straddle unit
    and workgroup boundaries, the table ends in a ragged unit, and the second call on the same index must find nothing left behind"""
    vdb, O = mods
    rng = np.random.default_rng(5)
    dim, n, nq = 128, 60011, 256  # (60011 = 1250 units + 11 rows)
    c = rng.standard_normal(dim).astype(np.float32)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[20010:20410] = c[None, :] + 0.3 * rng.standard_normal((400, dim)).astype(np.float32)
    base[n - 5:] = c[None, :] + 0.3 * rng.standard_normal((5, dim)).astype(np.float32)  # hits in the ragged last unit
    qs = (c[None, :] + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)
    oi, od, oc = O.flat_knn_batch(base, qs, 10, 0, nthreads=8)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        for coop in (0, 1):
            ix.set_param("flat_gemm8_coop", coop)
            for _ in range(2):
                idx, d, cnt = _both_forms(ix, qs, 10)
                _check_all(idx, d, cnt, oi, od, oc)
        assert (idx < n).all()
    finally:
        _reset(ix)
        ix.close()


def test_every_key_passes_and_the_spill_path(mods):
    """hub rows (row norms over decades) and thresholds made for 4096 hits per query on a 20 000-row table: a fifth of all keys pass, far
    more than a workgroup's hit buffer holds between two hand-overs, so keys go to the candidate lists directly (the spill path); queries
    far from the table, whose keys nearly tie, let (nearly) every key pass and overflow their lists -- another tier answers them"""
    vdb, O = mods
    rng = np.random.default_rng(33)
    dim, n, nq = 128, 20005, 140
    base = (rng.standard_normal((n, dim)) * np.exp(rng.normal(0, 1.0, (n, 1)))).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    qs[:12] *= np.float32(300.0)  # far away: every row at (nearly) the same distance
    qs[12:16] = 0
    oi, od, oc = O.flat_knn_batch(base, qs, 10, 0, nthreads=8)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.set_param("flat_i8_hits", 4096)
    try:
        for res in (0, 1):
            ix.set_param("flat_gemm8_res", res)
            idx, d, cnt = _both_forms(ix, qs, 10)
            _check_all(idx, d, cnt, oi, od, oc)
        print("hits per query: mean", ix.get_stat("flat_i8_hits_sum") / nq, "max", ix.get_stat("flat_i8_hits_max"), "passed on", ix.get_stat("flat_i8_redo"))
    finally:
        _reset(ix)
        ix.close()


def test_nothing_passes(mods):
    """flat_gemm_debug bit 0: thresholds of -inf, no key passes, the stage stays empty through every hand-over and the no-hit detection
    downstream must fire (every query handed on; the answers stay)"""
    vdb, O = mods
    rng = np.random.default_rng(8)
    n, dim, nq = 40000, 192, 96
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    oi, od, oc = O.flat_knn_batch(base, qs, 10, 0, nthreads=8)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.set_param("flat_gemm_debug", 1)
    try:
        for epi in FORMS:
            ix.set_param("flat_gemm8_epi", epi)
            ix.set_param("flat_i8_stats", 1)
            s0 = ix.get_stat("flat_i8_second_queries")
            idx, d, cnt = ix.flat_knn(qs, 10)
            _check_all(idx, d, cnt, oi, od, oc)
            assert ix.get_stat("flat_i8_hits_sum") == 0
            assert ix.get_stat("flat_i8_second_queries") - s0 == nq
    finally:
        ix.set_param("flat_gemm_debug", 0)
        _reset(ix)
        ix.close()


@pytest.mark.parametrize("n,nq", [(125000, 512), (125000, 256), (17000, 130)])
def test_small_blocks_and_waves_without_units(mods, n, nq):
    """125k rows: the cooperative form hands its buffer over every 3 units, so the stage is non-empty at most hand-overs (sets of 4 and 2);
    17 000 rows: 355 units on 360 waves, the last waves have none (they score a re-read unit whose rows are past n and must report nothing).
    Two calls each."""
    vdb, O = mods
    dim = 128
    rng = np.random.default_rng(n + nq)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    try:
        a = _both_forms(ix, qs, 10)
        if n >= 98304:
            assert ix.get_stat("flat_gemm8_coop_sets") == (4 if nq == 512 else 2)
        b = _both_forms(ix, qs, 10)
        _same(a, b)
        sel = rng.choice(nq, 40, replace=False)
        oi, od, oc = O.flat_knn_batch(base, qs[sel], 10, 0, nthreads=8)
        _check_all(a[0][sel], a[1][sel], a[2][sel], oi, od, oc)
        assert (a[0] < n).all()
    finally:
        _reset(ix)
        ix.close()


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_full_size_both_metrics(mods, dist):
    """1M x 960 with 256 queries (two groups: cooperative sets of 2), as tests/test_fullsize_gpu.py builds it: both epilogue forms give the
    same answers and hit counts, 16 queries are held against the oracle"""
    import torch

    from bench import gist_like_gpu

    vdb, O = mods
    N, DIM, K = 1_000_000, 960, 10
    dev = torch.device("cuda", 0)
    base = gist_like_gpu(torch, N, DIM, 1806, dev)
    qs = gist_like_gpu(torch, 256, DIM, 1807, dev).cpu().numpy()
    ix = vdb.GpuIndex(DIM, dist)
    ix.add_device(base.data_ptr(), N)
    try:
        idx, d, cnt = _both_forms(ix, qs, K)
        assert (cnt == K).all() and ix.get_stat("flat_gemm8_coop_sets") == 2 and ix.get_stat("flat_i8_queries") == 2 * len(qs)
        host = base.cpu().numpy()
        sel = np.arange(0, 256, 16)
        oi, od, oc = O.flat_knn_batch(host, qs[sel], K, O.L2SQR if dist == "l2sqr" else O.COSINE, nthreads=16)
        assert np.array_equal(idx[sel], oi) and np.array_equal(d[sel], od)
    finally:
        _reset(ix)
        ix.close()
        del base
        torch.cuda.empty_cache()


def test_the_switches_reject_what_they_cannot_run(mods):
    """flat_gemm8_epi takes 0 or 1; flat_gemm8_grid takes multiples of 32 (no silent rounding), and a grid whose workgroups per XCD the sets
    of a call do not divide is an error of that call, not a wrong answer"""
    vdb, O = mods
    rng = np.random.default_rng(2)
    n, dim, nq = 100000, 128, 1024  # 8 groups: sets of 8
    base = rng.standard_normal((n, dim)).astype(np.float32)
    qs = rng.standard_normal((nq, dim)).astype(np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        for bad in (2, -1):
            with pytest.raises(vdb.VdbError):
                ix.set_param("flat_gemm8_epi", bad)
        for bad in (16, 100, 224 + 8, 288):
            with pytest.raises(vdb.VdbError):
                ix.set_param("flat_gemm8_grid", bad)
        ref = ix.flat_knn(qs, 10)
        ix.set_param("flat_gemm8_grid", 192)  # 24 workgroups per XCD: three sets of 8
        _same(ref, ix.flat_knn(qs, 10))
        ix.set_param("flat_gemm8_grid", 224)  # 28 per XCD: no whole number of sets of 8 ...
        with pytest.raises(vdb.VdbError):
            ix.flat_knn(qs, 10)
        got = ix.flat_knn(qs[:512], 10)  # ... but seven sets of 4
        assert ix.get_stat("flat_gemm8_coop_sets") == 4
        for x, y in zip(got, ref):
            np.testing.assert_array_equal(x, y[:512])
    finally:
        ix.set_param("flat_gemm8_grid", 0)
        _reset(ix)
        ix.close()
