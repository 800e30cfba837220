"""GPU: BASELINE configs 3 (HNSW) and 4 (PQ-Flat), HNSW+PQ and IVF at the benchmark's full size (1,000,000 x 960, the bench's
low-rank gist-like rows and queries), against the CPU oracle: indices identical, distances bit for bit.

Paths that only come into play at this size: a graph of ~5 levels from the GPU-assisted builder at batch 1024 /
ef_construction 200, the walk's fp16 pre-pass (calls of >= 768 queries), the PQ quantised scans (candidate caps and a
sampled threshold that only bind when n is large; the 8-bit-code scan from n >= 65 536) and IVF with 1 000 clusters of ~1 000
rows.  Every check also asserts through get_stat / hnsw_last_stats that the path it names answered.  The hnsw_*, ivf_* and
pq_* settings are process-global: each test puts back the default it changed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, M_PQ = 1_000_000, 960, 320
THREADS = 16  # the CPUs a GPU job may use


@pytest.fixture(scope="module")
def world():
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_lowrank_gpu
    from oracle import oracle as O

    dev = torch.device("cuda", 0)
    base = gist_lowrank_gpu(torch, N, DIM, 1806, dev)
    qs = gist_lowrank_gpu(torch, 1024, DIM, 1807, dev).cpu().numpy()
    host = base.cpu().numpy()
    pool = ThreadPoolExecutor(THREADS)  # the oracle's ctypes calls release the GIL: one query per thread
    opened = []

    def index(dist="l2sqr", rows=N):
        ix = vdb.GpuIndex(DIM, dist)
        ix.add_device(base.data_ptr(), rows)
        opened.append(ix)
        return ix

    yield {"vdb": vdb, "O": O, "torch": torch, "base": base, "host": host, "qs": qs, "pool": pool, "index": index, "cache": {}}
    pool.shutdown()
    for ix in opened:
        ix.close()
    del base
    torch.cuda.empty_cache()


def _oracle(w, fn, rows, k):
    """fn(q) -> (idx, dist) of the oracle for each query row in `rows`, stacked as [len(rows), k] (padded like the library)"""
    r = list(w["pool"].map(fn, rows))
    oi = np.stack([np.pad(x[0], (0, k - len(x[0]))) for x in r]).astype(np.uint64)
    od = np.stack([np.pad(x[1], (0, k - len(x[1]))) for x in r]).astype(np.float32)
    return oi, od


def _same(got, exp, what=""):
    gi, gd = got[0], got[1]
    assert np.array_equal(np.asarray(gi).astype(np.uint64), exp[0]), what
    assert np.array_equal(gd, exp[1]), what


@pytest.fixture(scope="module")
def hnsw(world):
    w = world
    ix = w["index"]()
    ix.hnsw_build(M=16, ef_construction=200, seed=42, batch=1024, nthreads=THREADS)
    g = ix.hnsw_export()
    oh = w["O"].HNSW.from_graph(w["host"], 0, 16, 200, g)
    return ix, g, oh


@pytest.fixture(scope="module")
def pq4_cent(world):
    """the bench's PQ training: a second index over the first 10 000 rows, 4-bit codes, m = dim / 3"""
    tr = world["index"](rows=10_000)
    tr.pq_build(n_bits=4, m=M_PQ, max_iter=20, tol=1e-6, seed=42)
    return tr.pq_export()["centroids"]


def test_hnsw_graph_shape(world, hnsw):
    ix, g, oh = hnsw
    n, m, mm0 = g["n"], g["m"], g["max_m0"]
    assert n == N and m == 16 and mm0 == 32
    len0, vl = g["len0"].astype(np.int64), g["vec_level"].astype(np.int64)

    def check_lists(lists, lens, owners, cap, level):
        assert (lens <= cap).all(), level
        live = np.arange(cap)[None, :] < lens[:, None]
        ids = np.where(live, lists.astype(np.int64), -1)
        assert (ids[live] < n).all(), level
        assert not (live & (ids == owners[:, None])).any(), f"self-link at level {level}"
        s = np.sort(np.where(live, ids, n + np.arange(cap)[None, :]), axis=1)  # dead slots: distinct sentinels
        assert not (s[:, 1:] == s[:, :-1]).any(), f"duplicate id in a list at level {level}"
        assert (vl[ids[live]] >= level).all(), f"a link at level {level} to a node below it"

    assert (len0 >= 1).all()  # every node of a graph of > 1 nodes has a neighbour at level 0 (upper lists may be empty)
    check_lists(g["level0"].reshape(n, mm0), len0, np.arange(n), mm0, 0)
    up, ul = g["upper"].reshape(-1, m), g["upper_len"].astype(np.int64)
    assert len(ul) == vl.sum()
    owner = np.repeat(np.arange(n), vl)  # node-major: node i's lists for levels 1 .. vec_level[i]
    first = np.concatenate([[0], np.cumsum(vl)[:-1]])
    level = np.arange(len(ul)) - np.repeat(first, vl) + 1
    assert (level >= 1).all() and (level <= vl[owner]).all()
    for lev in range(1, int(vl.max()) + 1):
        sel = level == lev
        check_lists(up[sel], ul[sel], owner[sel], m, lev)
    top = int(vl.max())
    assert top >= 3  # ~log_16(1e6) levels
    assert g["has_enter"] == 1 and g["enter_level"] == top and vl[g["enter_point"]] == top


def test_hnsw_search_vs_oracle(world, hnsw):
    w = world
    ix, g, oh = hnsw
    qs = w["qs"]
    # (a) one call of all 1024 queries: the fp16 pre-pass runs (calls of >= 768 queries) and drops candidates
    a_i, a_d, a_c = ix.knn_with_ef(qs, 10, 128)
    stats = ix.hnsw_last_stats()
    dropped = ix.get_stat("hnsw_half_dropped")
    oi, od, oc, nd, ne = oh.knn_batch(qs, 10, 128, nthreads=THREADS)
    assert np.array_equal(a_i.astype(np.uint64), oi) and np.array_equal(a_d, od) and np.array_equal(a_c, oc)
    assert stats == (nd, ne), "distance-evaluation / expansion counts differ from the oracle"
    assert dropped > 0
    # (b) the same call without the pre-pass: byte for byte the same answer
    try:
        ix.set_param("hnsw_half", 0)
        b_i, b_d, b_c = ix.knn_with_ef(qs, 10, 128)
        assert ix.get_stat("hnsw_half_dropped") == 0
    finally:
        ix.set_param("hnsw_half", 1)
    assert a_i.tobytes() == b_i.tobytes() and a_d.tobytes() == b_d.tobytes() and a_c.tobytes() == b_c.tobytes()
    # (c) small calls at the extremes of k and ef (k = ef = 200: the builder's own search shape)
    q64 = qs[:64]
    for k, ef in ((10, 10), (10, 200), (100, 128), (200, 200)):
        gi, gd, gc = ix.knn_with_ef(q64, k, ef)
        oi, od, oc, nd, ne = oh.knn_batch(q64, k, ef, nthreads=THREADS)
        assert np.array_equal(gi.astype(np.uint64), oi) and np.array_equal(gd, od) and np.array_equal(gc, oc), (k, ef)
        assert ix.hnsw_last_stats() == (nd, ne), (k, ef)
    # (d) without the row staging (DMA) of the exact walk
    try:
        ix.set_param("hnsw_dma", 0)
        gi, gd, gc = ix.knn_with_ef(qs[64:128], 10, 128)
    finally:
        ix.set_param("hnsw_dma", 1)
    _same((gi, gd), (a_i[64:128].astype(np.uint64), a_d[64:128]), "dma off")
    # (e) a pool of one entry: every walk goes over to the heap walk
    try:
        ix.set_param("hnsw_pool_cap", 1)
        before = ix.get_stat("hnsw_heap_walk_queries")
        gi, gd, gc = ix.knn_with_ef(qs[128:144], 10, 128)
        moved = ix.get_stat("hnsw_heap_walk_queries") - before
    finally:
        ix.set_param("hnsw_pool_cap", 2048)
    assert moved > 0
    _same((gi, gd), (a_i[128:144].astype(np.uint64), a_d[128:144]), "heap walk")
    # (f) one-query calls equal their row of the 1024-query call
    for q in (0, 1, 511, 1023):
        gi, gd = ix.knn_with_ef(qs[q], 10, 128)
        assert gi.tolist() == a_i[q].tolist() and np.array_equal(gd, a_d[q]), q


def test_hnsw_pq_vs_oracle(world, hnsw, pq4_cent):
    """HNSWIndex::knn_pq on the full-size graph: ADC walk over GPU-encoded codes, exact re-sort"""
    w = world
    O = w["O"]
    ix, g, oh = hnsw
    ix.pq_attach(4, M_PQ, pq4_cent, None)
    try:
        qs = w["qs"][:64]
        gi, gd, gc = ix.knn_pq(qs, 10, 128)
        opq = O.PQ.from_centroids(DIM, M_PQ, 4, 0, pq4_cent)
        opq.set_codes(ix.pq_export()["codes"])
        exp = _oracle(w, lambda q: oh.knn_pq(opq, qs[q], 10, 128), range(len(qs)), 10)
        _same((gi, gd), exp, "hnsw knn_pq")
    finally:
        ix.pq_clear()


@pytest.fixture(scope="module")
def pq_flat(world, pq4_cent):
    ix = world["index"]()
    ix.pq_attach(4, M_PQ, pq4_cent, None)
    return ix


def test_pq_flat_4bit_l2(world, pq_flat, pq4_cent):
    """config 4: codes encoded on the GPU equal the oracle's encoder; one 1000-query call (the bench's step) of the quantised
    16-query scan (k_pq_adc16) equals FlatIndex::knn_pq on a sample that covers the first and last query of each group it touches"""
    w = world
    O, host, qs = w["O"], w["host"], w["qs"]
    ix = pq_flat
    codes = ix.pq_export()["codes"]
    opq = O.PQ.from_centroids(DIM, M_PQ, 4, 0, pq4_cent)
    rows = np.unique(np.concatenate([[0, N - 1], np.random.default_rng(5).choice(N, 4096, replace=False)]))
    enc = np.stack(list(w["pool"].map(lambda r: opq.encode_row(host[r]), rows)))
    assert np.array_equal(codes[rows], enc)
    opq.set_codes(codes)
    before, redo0 = ix.get_stat("pq_adc16_queries"), ix.get_stat("pq_adc16_redo")
    gi, gd, gc = ix.knn_pq(qs[:1000], 10, 100)
    assert ix.get_stat("pq_adc16_queries") == before + 1000
    assert ix.get_stat("pq_adc16_redo") == redo0  # the quantised scan answered every query: none handed to the f32 scan
    assert (gc == 10).all()
    sample = sorted({min(q, 999) for grp in (0, 1, 17, 30, 44, 51, 58, 61, 62) for q in (16 * grp, 16 * grp + 5, 16 * grp + 10, 16 * grp + 15)})
    assert len(sample) >= 32
    exp = _oracle(w, lambda q: O.flat_knn_pq(host, opq, qs[q], 10, 100), sample, 10)
    _same((gi[sample], gd[sample]), exp, "pq flat 4-bit")


def test_pq_flat_8bit_l2(world):
    """8-bit codes (256 centroids per group): the 16-queries-per-pass scan on sliced one-byte tables (k_pq_adc8x16, n >= 65 536)"""
    w = world
    O, host, qs = w["O"], w["host"], w["qs"]
    tr = w["index"](rows=20_000)
    tr.pq_build(n_bits=8, m=M_PQ, max_iter=5, tol=1e-6, seed=42)
    cent8 = tr.pq_export()["centroids"]
    ix = w["index"]()  # (its own index: the 4-bit table of the config-4 index stays as it is)
    ix.pq_attach(8, M_PQ, cent8, None)
    codes = ix.pq_export()["codes"]
    opq = O.PQ.from_centroids(DIM, M_PQ, 8, 0, cent8)
    rows = np.array([0, 1, N // 2, N - 1])
    assert np.array_equal(codes[rows], np.stack([opq.encode_row(host[r]) for r in rows]))
    opq.set_codes(codes)
    nq = 64
    a0 = ix.get_stat("pq_adc16_queries")
    h0 = ix.get_stat("pq_q8_overflow") + ix.get_stat("pq_q8_short")
    gi, gd, gc = ix.knn_pq(qs[:nq], 10, 100)
    assert ix.get_stat("pq_adc16_queries") > a0
    assert ix.get_stat("pq_q8_overflow") + ix.get_stat("pq_q8_short") - h0 < nq  # (the queries handed to the f32 scan)
    sample = list(range(0, nq, 4))
    exp = _oracle(w, lambda q: O.flat_knn_pq(host, opq, qs[q], 10, 100), sample, 10)
    _same((gi[sample], gd[sample]), exp, "pq flat 8-bit")


def test_pq_flat_4bit_cosine(world):
    w = world
    O, host, qs = w["O"], w["host"], w["qs"]
    tr = w["index"]("cosine", rows=10_000)
    tr.pq_build(n_bits=4, m=M_PQ, max_iter=20, tol=1e-6, seed=42)
    cent = tr.pq_export()["centroids"]
    ix = w["index"]("cosine")
    ix.pq_attach(4, M_PQ, cent, None)
    opq = O.PQ.from_centroids(DIM, M_PQ, 4, 1, cent)
    opq.set_codes(ix.pq_export()["codes"])
    before, redo0 = ix.get_stat("pq_adc16_queries"), ix.get_stat("pq_adc16_redo")
    gi, gd, gc = ix.knn_pq(qs[:64], 10, 100)
    assert ix.get_stat("pq_adc16_queries") == before + 64
    assert ix.get_stat("pq_adc16_redo") == redo0
    sample = [0, 9, 15, 16, 31, 40, 48, 63]
    exp = _oracle(w, lambda q: O.flat_knn_pq(host, opq, qs[q], 10, 100, O.COSINE), sample, 10)
    _same((gi[sample], gd[sample]), exp, "pq flat 4-bit cosine")


def test_ivf_full_size(world):
    """IVFIndex::from_vec_set as the bench builds it: 1000 clusters, k-means on 10 000 sampled rows, 10 iterations"""
    w = world
    O, host, qs = w["O"], w["host"], w["qs"]
    ix = w["index"]()
    ix.prof_enable(True)  # (the scan's tier statistics are kept by measurement calls)
    ix.ivf_build(1000, train_n=10000, max_iter=10, tol=1e-6, seed=42)
    ex = ix.ivf_export()
    cent, assign = ex["centroids"], ex["assign"]
    # assignment: the nearest centroid (find_nearest) of a 65 536-row sample, in 16 slices on the oracle
    sample = np.sort(np.random.default_rng(6).choice(N, 65536, replace=False))
    parts = list(w["pool"].map(lambda s: O.IVF(host[s], cent, O.L2SQR).assign, np.array_split(sample, THREADS)))
    assert np.array_equal(assign[sample], np.concatenate(parts))
    oiv = O.IVF(host, cent, O.L2SQR, assign=assign)
    q64 = qs[:64]
    for n_probes in (4, 32):
        exp = _oracle(w, lambda q: oiv.knn(q64[q], 10, n_probes), range(len(q64)), 10)
        for q8, half in ((2, 1), (1, 1), (0, 1), (1, 0)):
            try:
                ix.set_param("ivf_q8", q8)
                ix.set_param("ivf_half", half)
                gi, gd, gc = ix.ivf_knn(q64, 10, n_probes)
                offers, kept, kept_q8 = (ix.get_stat(s) for s in ("ivf_last_offers", "ivf_last_kept", "ivf_last_kept_q8"))
            finally:
                ix.set_param("ivf_q8", 1)
                ix.set_param("ivf_half", 1)
            _same((gi, gd), exp, (n_probes, q8, half))
            what = (n_probes, q8, half, offers, kept, kept_q8)
            if n_probes == 32 or not (q8 and half):  # (at 4 probes, ~4 000 offers per query, the 8-bit tier's lists of 1 024 may
                assert (kept_q8 > 0) == bool(q8 and half), what  # overflow: the call then goes on with the fp16 tier alone)
            if half:  # the fp16 tier answered: it passed on only part of the offers to the exact stage
                assert 0 < kept < offers, what
            else:  # the plain scan: every offer reaches the exact stage
                assert kept == offers > 0, what
