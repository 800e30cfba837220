"""GPU: one index of 4 500 000 x 960 rows, so that n * d = 4.32e9 > 2^32.  Row offsets pass 2^31 and 2^32 elements in the f32
rows, 2^32 bytes in the 8-bit images and 2^33 bytes in the fp16 images: every mirror builder and every kernel that reads rows by
id must form those offsets in 64 bits.  No host copy of the rows exists; the expected answer is known by construction:

- bulk rows: uniform [0, 1) with coordinate 0 shifted to [4, 5)  (all coordinates >= 0)
- queries and planted rows: every coordinate <= 0, coordinate 0 <= -0.1; a planted row is its anchor plus noise of ~1e-3
- so every bulk row is at L2Sqr >= 4.1^2 and at Cosine >= 1 (q . x <= 0) from every query, and the planted rows are far
  closer: the top-k over the whole index is the oracle's top-k over the planted rows alone, mapped to their global ids.

Planted rows sit on both sides of the rows where the byte / element offsets cross 2^30 / 2^31 / 2^32 (and at rows 0, 1, n-2,
n-1), so every answer mixes rows from below and above the boundaries.  Each run asserts through get_stat which tier answered."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, K = 4_500_000, 960, 10
ANCHORS, PER_ANCHOR, QPA = 16, 24, 8
BOUNDARIES = (2**30 // DIM, 2**31 // DIM, 2**32 // DIM)  # f32 bytes 2^32; elements / int8 bytes 2^31, 2^32 (fp16 bytes 2^33)


def _special_rows():
    rows = [0, 1, N - 2, N - 1]
    for b in BOUNDARIES:
        rows += [b - 1, b, b + 1]
    return sorted(rows)


@pytest.fixture(scope="module")
def world():
    import torch

    from oracle import oracle as O

    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(4500))
    g = torch.Generator(device=dev)
    g.manual_seed(4500)
    base = torch.rand((N, DIM), generator=g, device=dev, dtype=torch.float32)
    base[:, 0] += 4.0
    bulk_min0, bulk_min = float(base[:, 0].min()), float(base.min())

    anchors = -rng.uniform(0.01, 1.0, (ANCHORS, DIM)).astype(np.float32)
    anchors[:, 0] = -rng.uniform(0.2, 1.0, ANCHORS).astype(np.float32)

    def near(centres, scale):
        x = centres + rng.standard_normal(centres.shape).astype(np.float32) * np.float32(scale)
        x = np.minimum(x, np.float32(0.0))
        x[:, 0] = np.minimum(x[:, 0], np.float32(-0.1))
        return x.astype(np.float32)

    # queries: the anchor itself first, then the anchor plus ~1e-4 noise; nq = 16 takes the first of each anchor
    qs = near(np.repeat(anchors, QPA, axis=0), 1e-4)
    qs[::QPA] = anchors
    special = _special_rows()
    free = rng.choice(N, ANCHORS * PER_ANCHOR + 64, replace=False)
    free = [int(r) for r in free if r not in set(special)][: ANCHORS * PER_ANCHOR - len(special)]
    pos = np.array(special + free, dtype=np.int64)
    owner = np.concatenate([np.arange(len(special)),  # special row j belongs to anchor j (13 specials, 16 anchors)
                            np.repeat(np.arange(ANCHORS), [PER_ANCHOR - (j < len(special)) for j in range(ANCHORS)])])
    # the special rows sit closest to their anchor (noise 1e-4): each one is its anchor's queries' first answer
    planted = np.where((np.arange(len(pos)) < len(special))[:, None], near(anchors[owner], 1e-4), near(anchors[owner], 1e-3))
    order = np.argsort(pos)
    pos, owner, planted = pos[order], owner[order], np.ascontiguousarray(planted[order])
    assert np.bincount(owner, minlength=ANCHORS).tolist() == [PER_ANCHOR] * ANCHORS
    base[torch.from_numpy(pos).to(dev)] = torch.from_numpy(planted).to(dev)
    torch.cuda.synchronize()

    # the margin, in float64: no bulk row can be among the top-K planted rows of any query
    assert bulk_min >= 0.0 and bulk_min0 >= 4.0
    assert float(qs.max()) <= 0.0 and float(qs[:, 0].max()) <= -0.1
    lb_l2 = (bulk_min0 - float(qs[:, 0].max())) ** 2
    assert lb_l2 >= 16.8
    q64, p64 = qs.astype(np.float64), planted.astype(np.float64)
    d_l2 = (q64 * q64).sum(1)[:, None] + (p64 * p64).sum(1)[None, :] - 2.0 * q64 @ p64.T
    d_cos = 1.0 - (q64 @ p64.T) / np.sqrt((q64 * q64).sum(1)[:, None] * (p64 * p64).sum(1)[None, :])
    assert np.sort(d_l2, axis=1)[:, K - 1].max() < 0.01 * lb_l2
    assert np.sort(d_cos, axis=1)[:, K - 1].max() < 0.01  # bulk rows: >= 1
    expect = {}
    for kind in (O.L2SQR, O.COSINE):
        oi, od, oc = O.flat_knn_batch(planted, qs, K, kind, nthreads=16)
        assert (oc == K).all()
        expect[kind] = (pos[oi.astype(np.int64)].astype(np.uint64), od)
    # the queries' first answers include rows past every boundary
    first = expect[O.L2SQR][0][::QPA, 0]
    for b in BOUNDARIES:
        assert (first > b).any() and (first < b).any()
    yield torch, base, anchors, qs, pos, special, expect
    del base
    torch.cuda.empty_cache()


def _check(got, exp, sel, what):
    gi, gd, gc = got
    ei, ed = exp
    assert (np.asarray(gc) == K).all(), what
    assert np.array_equal(np.asarray(gi).astype(np.uint64), ei[sel]), what
    assert np.array_equal(gd, ed[sel]), what


# (name, set_param values, counter that must advance by the call's queries, counters that must not move).  No query may be
# handed on: the redo counters of the 8-bit and fp16 tiers stay put, and so does the exact-scan fallback behind split-bf16.
STILL = ("flat_i8_redo", "flat_half_redo", "flat_fallback")
TIERS = (
    ("8-bit", {"flat_i8": 2, "flat_half": 0, "flat_i8_refine": 1}, "flat_i8_queries", ("flat_half_queries",) + STILL),
    ("fp16", {"flat_i8": 1, "flat_half": 2, "flat_i8_refine": 1}, "flat_half_queries", ("flat_i8_queries",) + STILL),
    ("split-bf16", {"flat_i8": 1, "flat_half": 1, "flat_i8_refine": 1}, None, ("flat_i8_queries", "flat_half_queries") + STILL),
)


@pytest.mark.parametrize("dist,kind", [("l2sqr", 0), ("cosine", 1)])
def test_flat_tiers_past_4gib(world, dist, kind):
    """Every Flat tier on the same index: the 8-bit pass (k_tile_rows_i8), the fp16 pass (fp16 tile image), split-bf16
    (k_tile_rows), the key refinement from the row-major fp16 image, the exact scan and flat_knn_device on torch tensors."""
    import lab_1806_vec_db_amd as vdb

    torch, base, anchors, qs, pos, special, expect = world
    exp = expect[kind]
    ix = vdb.GpuIndex(DIM, dist)
    try:
        ix.add_device(base.data_ptr(), N)
        assert len(ix) == N
        for name, params, counter, still in TIERS:
            for p, v in params.items():
                ix.set_param(p, v)
            for nq, sel in ((ANCHORS, slice(None, None, QPA)), (ANCHORS * QPA, slice(None))):
                c0 = ix.get_stat(counter) if counter else 0
                s0 = [ix.get_stat(s) for s in still]
                _check(ix.flat_knn(qs[sel], K), exp, sel, (name, nq))
                if counter:
                    assert ix.get_stat(counter) == c0 + nq, (name, nq)
                assert [ix.get_stat(s) for s in still] == s0, (name, nq)
            if name == "split-bf16":
                assert ix.get_stat("flat_bf16_mirror") == 1
        # the 8-bit pass with its hit keys refined from the row-major fp16 image (calls of >= 64 queries)
        ix.set_param("flat_i8", 2)
        ix.set_param("flat_i8_refine", 2)
        r0, q0 = ix.get_stat("flat_i8_refine_queries"), ix.get_stat("flat_i8_queries")
        s0 = [ix.get_stat(s) for s in STILL]
        _check(ix.flat_knn(qs, K), exp, slice(None), "refine")
        assert ix.get_stat("flat_i8_refine_queries") == r0 + len(qs) and ix.get_stat("flat_i8_queries") == q0 + len(qs)
        assert [ix.get_stat(s) for s in STILL] == s0
        for p in ("flat_i8", "flat_half", "flat_i8_refine"):
            ix.set_param(p, 0)
        # the strict-order exact scan over the f32 rows
        ix.set_flat_mode(1)
        sel = slice(None, None, QPA)
        _check(ix.flat_knn(qs[sel], K), exp, sel, "exact")
        ix.set_flat_mode(0)
        # flat_knn_device: queries and outputs are torch tensors on the device
        dq = torch.from_numpy(qs).to(base.device)
        o_idx = torch.zeros((len(qs), K), dtype=torch.int64, device=base.device)
        o_dist = torch.zeros((len(qs), K), dtype=torch.float32, device=base.device)
        o_cnt = torch.zeros((len(qs),), dtype=torch.int64, device=base.device)
        ix.flat_knn_device(dq.data_ptr(), len(qs), K, o_idx.data_ptr(), o_dist.data_ptr(), o_cnt.data_ptr())
        torch.cuda.synchronize()
        _check((o_idx.cpu().numpy(), o_dist.cpu().numpy(), o_cnt.cpu().numpy()), exp, slice(None), "device")
        assert ix.flat_fallback_count() == 0
    finally:
        ix.close()
        torch.cuda.empty_cache()


def test_ivf_past_4gib(world):
    """IVF on the same rows: the library assigns every row on the GPU (ivf_attach without an assignment), the 8-bit tier (its
    cluster-major and pair-major forms), the fp16 tier and the plain rerank read rows by id past 2^32 elements / bytes."""
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O

    torch, base, anchors, qs, pos, special, expect = world
    rng = np.random.Generator(np.random.PCG64(4501))
    bulk_c = (0.5 + rng.uniform(-0.05, 0.05, (16, DIM))).astype(np.float32)
    bulk_c[:, 0] += 4.0
    cent = np.ascontiguousarray(np.concatenate([anchors, bulk_c]), dtype=np.float32)
    ix = vdb.GpuIndex(DIM, "l2sqr")
    try:
        ix.add_device(base.data_ptr(), N)
        ix.prof_enable(True)  # (the scan's tier statistics are kept by measurement calls)
        ix.ivf_attach(cent)
        assign = ix.ivf_export()["assign"]
        # assignment of the planted rows and of the bulk rows around every boundary and at both ends
        near_b = [r for b in BOUNDARIES for r in range(b - 8, b + 9)] + list(range(8)) + list(range(N - 8, N))
        chk = np.unique(np.concatenate([pos, np.array(near_b, dtype=np.int64)]))
        rows = base[torch.from_numpy(chk).to(base.device)].cpu().numpy()
        assert np.array_equal(assign[chk], O.IVF(rows, cent, O.L2SQR).assign)
        # every query's nearest 16 centroids are the anchors, far ahead of the bulk centroids: at n_probes <= 16 only the anchors'
        # clusters are probed, and their rows (gathered in id order) are all the oracle needs
        cd = ((qs.astype(np.float64)[:, None, :] - cent.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        assert cd[:, :ANCHORS].max() < 0.5 * cd[:, ANCHORS:].min()
        ids = np.nonzero(assign < ANCHORS)[0]
        assert 0 < len(ids) <= 4096, len(ids)
        assert (ids > BOUNDARIES[-1]).any()
        sub = base[torch.from_numpy(ids).to(base.device)].cpu().numpy()
        oiv = O.IVF(sub, cent, O.L2SQR, assign=assign[ids])
        for n_probes in (4, 16):
            exp_i = np.zeros((len(qs), K), dtype=np.uint64)
            exp_d = np.zeros((len(qs), K), dtype=np.float32)
            for q in range(len(qs)):
                oi, od = oiv.knn(qs[q], K, n_probes)
                assert len(oi) == K
                exp_i[q], exp_d[q] = ids[oi.astype(np.int64)], od
            for q8, half in ((2, 1), (1, 1), (0, 1), (1, 0)):
                try:
                    ix.set_param("ivf_q8", q8)
                    ix.set_param("ivf_half", half)
                    _check(ix.ivf_knn(qs, K, n_probes), (exp_i, exp_d), slice(None), (n_probes, q8, half))
                    offers, kept, kept_q8, fetched = (ix.get_stat(s) for s in ("ivf_last_offers", "ivf_last_kept", "ivf_last_kept_q8",
                                                                               "ivf_last_rows_fetched_q8"))
                    what = (n_probes, q8, half, offers, kept, kept_q8, fetched)
                    assert (kept_q8 > 0) == (q8 != 0 and half != 0), what
                    # the cluster-major form of the 8-bit tier reads the probed clusters' rows once each; the pair-major form
                    # (ivf_q8 = 2) reads them per offer and fetches nothing of its own
                    assert (fetched > 0) == (q8 == 1 and half != 0), what
                    if half:  # the fp16 tier answered: it passed on only part of the offers to the exact stage
                        assert 0 < kept < offers, what
                    else:  # the plain scan: every offer reaches the exact stage
                        assert kept == offers > 0, what
                finally:
                    ix.set_param("ivf_q8", 1)
                    ix.set_param("ivf_half", 1)
    finally:
        ix.close()
        torch.cuda.empty_cache()
