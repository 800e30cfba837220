"""GPU: the multi-GPU context (vdb_ctx_* / vdb_sharded_*, csrc/ctx.hip) with MORE THAN ONE shard on one GPU.

VDB_CTX_LOOPBACK=1 lets vdb_ctx_create take the same device S times: S ranks, S local shards, no communicator, and the all-gather done
with device copies.  Everything else is the code a real S-GPU single-process context runs: the row partition and the global id offsets,
the exchange block layouts read at stride `block`, the k-NN and PQ merges over S gathered blocks, the replica query split (empty blocks
included) and its concatenation, the per-shard host threads, the mirroring of an HNSW graph / of IVF clusters to the other replicas.

Every comparison is bit for bit (ids, float32 bit patterns of the distances, counts) against the CPU oracle on the UNSHARDED rows and
against a plain GpuIndex over them.  The range search's many-shard cases live in test_sharded_range_gpu.py."""
import threading

import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

KIND = {"l2sqr": 0, "cosine": 1}
N, DIM = 6007, 64  # N % S != 0 for S in 2, 3, 5, 8; S = 8: seven shards of 751 rows and one of 750
NQ = 33            # odd: with k = 1 the [ids | distances] part of an exchange block is no multiple of 8 bytes before its padding


def _blocks(n, S):
    per = -(-n // S)
    return [(min(n, r * per), min(n, (r + 1) * per)) for r in range(S)]


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)


def _same(got, exp, what):
    """(idx, dist, cnt) equal bit for bit, slots beyond the count included"""
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], np.asarray(exp[0], dtype=np.uint64)), (what, "ids")
    assert got[1].dtype == np.float32 and np.array_equal(_bits(got[1]), _bits(exp[1])), (what, "distances")
    assert np.array_equal(got[2], np.asarray(exp[2], dtype=np.uint64)), (what, "counts")


def _same_lists(got, lists, what):
    """rows of (idx, dist, cnt) against per-query oracle lists (ids, distances) of length <= k; the slots beyond stay zero"""
    gi, gd, gc = got
    assert len(lists) == len(gi), what
    for q, (oi, od) in enumerate(lists):
        c = len(oi)
        assert int(gc[q]) == c, (what, q, int(gc[q]), c)
        assert gi[q, :c].tolist() == oi.tolist(), (what, q)
        assert np.array_equal(_bits(gd[q, :c]), _bits(od)), (what, q)
        assert not gi[q, c:].any() and not _bits(gd[q, c:]).any(), (what, q, "slots beyond the count")


def _loopback(monkeypatch, S, dist="l2sqr", dim=DIM):
    from lab_1806_vec_db_amd.sharded import ShardedIndex

    monkeypatch.setenv("VDB_CTX_LOOPBACK", "1")
    monkeypatch.delenv("VDB_CTX_FORCE_RCCL", raising=False)
    sh = ShardedIndex(dim, dist, devices=[0] * S)
    assert sh.info() == {"world": S, "n_local": S, "first_rank": 0, "has_comm": False}
    return sh


def _plain(base, dist):
    import lab_1806_vec_db_amd as vdb

    ref = vdb.GpuIndex(base.shape[1], dist)
    if len(base):
        ref.batch_add(base)
    return ref


@pytest.fixture(scope="module")
def big():
    """6007 x 64 with exact duplicates of rows 0..9 in the middle and of rows 5..7 at the end: for S >= 2 the copies lie in other shards
    than the originals, so a merged list must break distance ties by GLOBAL id across shards; queries 0..2 ARE such rows"""
    from oracle import oracle as O

    base = gist_like(N, dim=DIM, seed=301)
    base[N // 2:N // 2 + 10] = base[:10]
    base[N - 3:] = base[5:8]
    qs = gist_like(NQ, dim=DIM, seed=302)
    qs[0], qs[1], qs[2] = base[6], base[2], base[7]
    full = {}
    for dist, kind in KIND.items():
        oi, od, oc = O.flat_knn_batch(base, qs, 1024, kind, nthreads=16)
        assert (oc == 1024).all()
        assert oi[0, :3].tolist() == [6, N // 2 + 6, N - 2] and len(set(_bits(od[0, :3]).tolist())) == 1  # the tie, in id order
        assert oi[1, :2].tolist() == [2, N // 2 + 2] and oi[2, :3].tolist() == [7, N // 2 + 7, N - 1]
        full[dist] = (oi, od)
    return base, qs, full


@pytest.fixture(scope="module")
def tiny():
    """300 rows: at S = 8 every shard holds 38 rows or fewer, below k = 100; 5 rows: at S = 8 ranks 5..7 hold none"""
    base = gist_like(300, dim=DIM, seed=303)
    base[290:293] = base[1:4]  # ties across the first and the last shard
    return base, base[:5].copy(), gist_like(9, dim=DIM, seed=304)


def _oracle_topk(full, k):
    oi, od = full  # a top-k under a total order is the prefix of the top-1024
    return oi[:, :k], od[:, :k], np.full(len(oi), k, dtype=np.uint64)


# ---- ROWS layout, Flat ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 5, 8])
@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_rows_flat_knn_many_shards(big, dist, S, monkeypatch):
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O

    base, qs, full = big
    sh = _loopback(monkeypatch, S, dist)
    ref = _plain(base, dist)
    try:
        sh.set_rows(base)
        assert sh.layout == "rows" and len(sh) == N and not sh.poisoned
        # the partition: block lengths, and a local search answers with global ids
        for i, (r0, r1) in enumerate(_blocks(N, S)):
            loc = sh.local_index(i)
            assert len(loc) == r1 - r0, (i, len(loc), r0, r1)
            got = loc.flat_knn(qs[:4], 3)
            lists = [O.flat_knn(base[r0:r1], q, 3, KIND[dist]) for q in qs[:4]]
            _same_lists(got, [(oi + np.uint64(r0), od) for oi, od in lists], ("local", S, i))
        for k in (1, 10, 100, 1024):
            got = sh.flat_knn(qs, k)
            _same(got, _oracle_topk(full[dist], k), (dist, S, k, "oracle"))
            _same(got, ref.flat_knn(qs, k), (dist, S, k, "plain index"))
        _same(sh.flat_knn(qs[5], 10), _oracle_topk((full[dist][0][5:6], full[dist][1][5:6]), 10), "one query")
        gi, gd, gc = sh.flat_knn(qs, 0)
        assert gi.shape == (NQ, 0) and gc.tolist() == [0] * NQ
        with pytest.raises(vdb.VdbError, match="k must be <= 1024"):
            sh.flat_knn(qs, 1025)
        assert not sh.poisoned
        _same(sh.flat_knn(qs, 10), _oracle_topk(full[dist], 10), "after the refused k")
    finally:
        ref.close()
        sh.close()


@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_rows_flat_knn_short_and_empty_shards(tiny, dist, monkeypatch):
    from oracle import oracle as O

    t300, t5, qs = tiny
    S = 8
    for base, ks in ((t300, (100,)), (t5, (3, 10))):
        n = len(base)
        sh = _loopback(monkeypatch, S, dist)
        ref = _plain(base, dist)
        try:
            sh.set_rows(base)
            blocks = _blocks(n, S)
            assert [len(sh.local_index(i)) for i in range(S)] == [b - a for a, b in blocks]
            if n == 5:
                assert blocks[4] == (4, 5) and blocks[5:] == [(5, 5)] * 3  # ranks 5..7 hold no rows
            else:
                assert max(b - a for a, b in blocks) == 38
            for k in ks:
                got = sh.flat_knn(qs, k)
                _same_lists(got, [O.flat_knn(base, q, k, KIND[dist]) for q in qs], (dist, n, k, "oracle"))
                _same(got, ref.flat_knn(qs, k), (dist, n, k, "plain index"))
                assert got[2].tolist() == [min(k, n)] * len(qs)
        finally:
            ref.close()
            sh.close()


def test_rows_flat_knn_more_queries_than_one_exchange_chunk(big, monkeypatch):
    from oracle import oracle as O

    base, _, _ = big
    nq = 8200  # the exchange runs in chunks of 8192 queries
    many = gist_like(nq, dim=DIM, seed=305)
    sh = _loopback(monkeypatch, 3)
    ref = _plain(base, "l2sqr")
    try:
        sh.set_rows(base)
        got = sh.flat_knn(many, 10)
        _same(got, ref.flat_knn(many, 10), "plain index")
        pick = [0, 8191, 8192, 8199]
        _same_lists(tuple(a[pick] for a in got), [O.flat_knn(base, many[q], 10) for q in pick], "oracle")
    finally:
        ref.close()
        sh.close()


# ---- ROWS layout, PQ-Flat -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pq_refs(big):
    """per metric: the plain index with a trained PQ table, its export, the oracle's table over the same centroids and codes"""
    from oracle import oracle as O

    base, _, _ = big
    out = {}
    for dist, kind in KIND.items():
        ref = _plain(base, dist)
        ref.pq_build(n_bits=4, m=16, train_n=1500, max_iter=4, seed=3)
        pq = ref.pq_export()
        opq = O.PQ.from_centroids(DIM, 16, 4, kind, pq["centroids"])
        opq.set_codes(pq["codes"])
        out[dist] = (ref, pq, opq)
    yield out
    for ref, _, _ in out.values():
        ref.close()


@pytest.mark.parametrize("S", [2, 5, 8])
@pytest.mark.parametrize("dist", ["l2sqr", "cosine"])
def test_rows_knn_pq_many_shards(big, tiny, pq_refs, dist, S, monkeypatch):
    from oracle import oracle as O

    base, qs, _ = big
    qs = qs[:12]
    ref, pq, opq = pq_refs[dist]
    sh = _loopback(monkeypatch, S, dist)
    try:
        sh.set_rows(base)
        sh.pq_attach(4, 16, pq["centroids"])
        cases = [(10, 64), (5, 5), (10, 1500)]  # the last: past the register-resident select
        if S == 8:
            cases.append((10, 900))  # ef above the 751 rows of a shard: every shard's list is padded
        for k, ef in cases:
            got = sh.knn_pq(qs, k, ef)
            _same(got, ref._search(ref._lib.vdb_flat_knn_pq, qs, k, ef), (dist, S, k, ef, "plain index"))
            _same_lists(got, [O.flat_knn_pq(base, opq, q, k, ef, KIND[dist]) for q in qs], (dist, S, k, ef, "oracle"))
        gi, gd, gc = sh.knn_pq(qs, 0, 16)
        assert gc.tolist() == [0] * len(qs)
    finally:
        sh.close()
    # short shards (300 rows) and empty ones (5 rows) at S = 8, under the same centroids
    for small in tiny[:2]:
        n = len(small)
        sh = _loopback(monkeypatch, 8, dist)
        sref = _plain(small, dist)
        try:
            sh.set_rows(small)
            sh.pq_attach(4, 16, pq["centroids"])  # (an empty shard takes the table and contributes an empty list)
            sref.pq_attach(4, 16, pq["centroids"])
            spq = O.PQ.from_centroids(DIM, 16, 4, KIND[dist], pq["centroids"])
            spq.set_codes(sref.pq_export()["codes"])
            for k, ef in ((10, 64), (5, 5)):
                got = sh.knn_pq(tiny[2], k, ef)
                _same(got, sref._search(sref._lib.vdb_flat_knn_pq, tiny[2], k, ef), (dist, n, k, ef, "plain index"))
                _same_lists(got, [O.flat_knn_pq(small, spq, q, k, ef, KIND[dist]) for q in tiny[2]], (dist, n, k, ef, "oracle"))
                assert got[2].tolist() == [min(k, n)] * len(tiny[2])
        finally:
            sref.close()
            sh.close()


# ---- REPLICA layout -------------------------------------------------------------------------------------------------------------------
RN = 3000
NQS = (1, 2, 7, 77)  # S = 8: 2 queries leave six ranks with an empty block; S = 3: 77 = 26 + 26 + 25


@pytest.fixture(scope="module")
def replica_table():
    from oracle import oracle as O

    base = gist_like(RN, dim=DIM, seed=311)
    base[RN // 2:RN // 2 + 4] = base[:4]
    qs = gist_like(77, dim=DIM, seed=312)
    qs[0] = base[1]
    flat = {dist: O.flat_knn_batch(base, qs, 1500, kind, nthreads=16) for dist, kind in KIND.items()}
    return base, qs, flat


@pytest.mark.parametrize("S,dist", [(2, "l2sqr"), (3, "l2sqr"), (3, "cosine"), (8, "l2sqr")])
def test_replica_layout_many_replicas(replica_table, S, dist, monkeypatch):
    from lab_1806_vec_db_amd.sharded import replica_query_block
    from oracle import oracle as O

    base, qs, flat = replica_table
    kind = KIND[dist]
    assert [replica_query_block(2, 8, r) for r in range(8)] == [(0, 1), (1, 2)] + [(2, 2)] * 6
    assert [replica_query_block(77, 3, r) for r in range(3)] == [(0, 26), (26, 52), (52, 77)]
    sh = _loopback(monkeypatch, S, dist)
    ref = _plain(base, dist)
    try:
        sh.set_rows_replica(base)
        assert sh.layout == "replica" and len(sh) == RN
        assert [len(sh.local_index(i)) for i in range(S)] == [RN] * S
        # Flat: no merge in this layout, any k
        oi, od, oc = flat[dist]
        for nq in NQS:
            _same(sh.flat_knn(qs[:nq], 10), (oi[:nq, :10], od[:nq, :10], np.full(nq, 10)), (S, nq, "flat 10"))
            _same(sh.flat_knn(qs[:nq], 1500), (oi[:nq], od[:nq], oc[:nq]), (S, nq, "flat 1500"))
        _same(sh.flat_knn(qs, 10), ref.flat_knn(qs, 10), "plain index")
        # PQ-Flat
        ref.pq_build(n_bits=4, m=16, train_n=1000, max_iter=3, seed=3)
        pq = ref.pq_export()
        sh.pq_attach(4, 16, pq["centroids"])
        opq = O.PQ.from_centroids(DIM, 16, 4, kind, pq["centroids"])
        opq.set_codes(pq["codes"])
        for i in (0, S - 1):
            assert np.array_equal(sh.local_index(i).pq_export()["codes"], pq["codes"]), i
        exp = [O.flat_knn_pq(base, opq, q, 5, 40, kind) for q in qs]
        for nq in NQS:
            _same_lists(sh.knn_pq(qs[:nq], 5, 40), exp[:nq], (S, nq, "knn_pq"))
        _same(sh.knn_pq(qs, 5, 40), ref._search(ref._lib.vdb_flat_knn_pq, qs, 5, 40), "knn_pq, plain index")
        # HNSW: built on the first replica and mirrored to the others
        sh.hnsw_build(M=8, ef_construction=60, seed=5, batch=1, nthreads=1)
        g = sh.local_index(0).hnsw_export()
        g_last = sh.local_index(S - 1).hnsw_export()
        assert g.keys() == g_last.keys()
        for key in g:
            assert np.array_equal(g[key], g_last[key]), ("graph of the last replica", key)
        oh = O.HNSW.from_graph(base, kind, 8, 60, g)
        hi, hd, hc, _, _ = oh.knn_batch(qs, 10, 50)
        exp_pq = [oh.knn_pq(opq, q, 5, 40) for q in qs]
        for nq in NQS:
            _same(sh.knn_with_ef(qs[:nq], 10, 50), (hi[:nq], hd[:nq], hc[:nq]), (S, nq, "hnsw"))
            _same_lists(sh.hnsw_knn_pq(qs[:nq], 5, 40), exp_pq[:nq], (S, nq, "hnsw + pq"))
        # the same graph attached from arrays onto fresh replicas
        sh2 = _loopback(monkeypatch, S, dist)
        try:
            sh2.set_rows_replica(base)
            sh2.hnsw_attach(8, 60, g)
            g2 = sh2.local_index(S - 1).hnsw_export()
            for key in g:
                assert np.array_equal(g[key], g2[key]), ("attached graph of the last replica", key)
            for nq in (2, 77):
                _same(sh2.knn_with_ef(qs[:nq], 10, 50), (hi[:nq], hd[:nq], hc[:nq]), (S, nq, "attached hnsw"))
        finally:
            sh2.close()
        # IVF: clusters built on the first replica and mirrored
        sh.ivf_build(9, train_n=500, max_iter=3, seed=4)
        iv = sh.local_index(0).ivf_export()
        iv_last = sh.local_index(S - 1).ivf_export()
        assert np.array_equal(_bits(iv["centroids"]), _bits(iv_last["centroids"])) and np.array_equal(iv["assign"], iv_last["assign"])
        oivf = O.IVF(base, iv["centroids"], kind, assign=iv["assign"])
        for n_probes in (0, 3):
            exp = [oivf.knn(q, 10, n_probes or 4) for q in qs]
            for nq in NQS:
                _same_lists(sh.ivf_knn(qs[:nq], 10, n_probes), exp[:nq], (S, nq, "ivf", n_probes))
    finally:
        ref.close()
        sh.close()


@pytest.mark.parametrize("S", [3, 8])
def test_replica_counts_land_at_their_query_rows(S, monkeypatch):
    """a table smaller than k: Flat counts 40 everywhere; one IVF probe returns the size of the probed cluster, which differs from
    query to query, so a count copied to the wrong query row shows"""
    from oracle import oracle as O

    base = gist_like(40, dim=DIM, seed=321)
    qs = gist_like(7, dim=DIM, seed=322)
    sh = _loopback(monkeypatch, S)
    try:
        sh.set_rows_replica(base)
        got = sh.flat_knn(qs, 50)
        _same_lists(got, [O.flat_knn(base, q, 50) for q in qs], "flat, k > n")
        assert got[2].tolist() == [40] * 7
        sh.ivf_build(6, max_iter=3, seed=4)
        iv = sh.local_index(S - 1).ivf_export()
        oivf = O.IVF(base, iv["centroids"], 0, assign=iv["assign"])
        exp = [oivf.knn(q, 50, 1) for q in qs]
        assert len({len(oi) for oi, _ in exp}) > 1  # the counts differ between the queries
        _same_lists(sh.ivf_knn(qs, 50, 1), exp, "ivf, one probe")
    finally:
        sh.close()


def test_replica_more_queries_than_one_exchange_chunk(tiny, monkeypatch):
    """the replica exchange runs in chunks of 65536 queries: the second chunk's blocks land behind the first's"""
    from oracle import oracle as O

    base = tiny[0]
    nq = 65536 + 70
    many = gist_like(nq, dim=DIM, seed=323)
    sh = _loopback(monkeypatch, 3)
    ref = _plain(base, "l2sqr")
    try:
        sh.set_rows_replica(base)
        got = sh.flat_knn(many, 3)
        oi, od, oc = O.flat_knn_batch(base, many, 3, 0, nthreads=16)
        _same(got, (oi, od, oc), "oracle")
        _same(got, ref.flat_knn(many, 3), "plain index")
    finally:
        ref.close()
        sh.close()


# ---- host threads, argument rules -----------------------------------------------------------------------------------------------------
def test_two_threads_each_on_its_own_sharded_index(big, monkeypatch):
    base, qs, full = big
    shs = [_loopback(monkeypatch, 3) for _ in range(2)]
    try:
        for sh in shs:
            sh.set_rows(base)
        serial = shs[0].flat_knn(qs, 10)
        _same(serial, _oracle_topk(full["l2sqr"], 10), "serial")
        out, errs = [None] * 2, []
        bar = threading.Barrier(2)

        def work(t):
            try:
                bar.wait()
                for _ in range(3):
                    out[t] = shs[t].flat_knn(qs, 10)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errs, errs
        for t in range(2):
            _same(out[t], serial, ("thread", t))
    finally:
        for sh in shs:
            sh.close()


def test_loopback_argument_rules(monkeypatch):
    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.sharded import ShardedIndex

    monkeypatch.delenv("VDB_CTX_LOOPBACK", raising=False)
    monkeypatch.delenv("VDB_CTX_FORCE_RCCL", raising=False)
    with pytest.raises(vdb.VdbError, match="a device may appear once"):
        ShardedIndex(8, "l2sqr", devices=[0, 0])
    monkeypatch.setenv("VDB_CTX_LOOPBACK", "0")  # only "1" switches it on
    with pytest.raises(vdb.VdbError, match="a device may appear once"):
        ShardedIndex(8, "l2sqr", devices=[0, 0])
    for S in (1, 2, 8):
        sh = _loopback(monkeypatch, S, dim=8)
        sh.close()
    with pytest.raises(vdb.VdbError, match="device id out of range"):
        ShardedIndex(8, "l2sqr", devices=[0, 99])  # every other check stays
    monkeypatch.setenv("VDB_CTX_FORCE_RCCL", "1")
    with pytest.raises(vdb.VdbError, match="exclude each other"):
        ShardedIndex(8, "l2sqr", devices=[0, 0])
    with pytest.raises(vdb.VdbError, match="exclude each other"):
        ShardedIndex(8, "l2sqr", devices=[0])
    monkeypatch.delenv("VDB_CTX_FORCE_RCCL")
    sh = ShardedIndex(8, "l2sqr", device=0, rank=0, world=1)  # vdb_ctx_create_rank does not look at the variable
    assert sh.info() == {"world": 1, "n_local": 1, "first_rank": 0, "has_comm": False}
    sh.close()
