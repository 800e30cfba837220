"""GPU: SEQUENCES of row edits on one Flat index against the host model (tests/edit_model.py), on every Flat tier.

The per-feature tests apply one edit to a freshly prepared index.  The states only a sequence produces -- a mirror that shrank and then
grew past its old extent, a mirror behind the table when a remove / update arrives, a stale (too coarse) fp16 scale that later patches
run under, gathered-row images extended after they were invalidated, label columns that shrank and grew -- are reached here.  After every
write, queries are aimed at what the write touched (new vectors, OLD vectors, rows moved into holes, the ragged last tile, tile 0): a stale
16-row tile, norm or label changes the answer only there.  Every check is bit for bit against the CPU oracle on the model's rows: ids,
distances as uint32, counts.  A forced-tier search also asserts its tier's counter, so a silent fall-back to the exact scan fails.

Tiers are forced as in test_update_rows_gpu.py: set_flat_mode(2) with (flat_i8, flat_half) = i8 (2, 0), fp16 (1, 2), bf16 (1, 1).
flat_i8 = 1 switches the 8-bit tier OFF: then add_rows extends the fp16 mirror at once; with flat_i8 = 0 / 2 (Index::i8_defers_half) it
waits for its first use, and a remove / update that finds it behind drops it.

Shapes: 22 037 rows x 128 (= 16 * 1377 + 5 = 192 * 114 + 149), the shape of the existing edit tests; 1003 rows for the small-table paths
(one-launch kernel, scan); the seeded sequences start from 3011 / 9005 / 17 003 rows (across the 16 384-row switch of the unforced mode)
with dim 64 / 128 / 192.  dim 64 is one 64-wide k block: the 8-bit and fp16 filter kernels need two, so only the split-bf16 tier is forced
there.  48 queries per check, k = 7.

What these sequences cannot see: rows at or past n that stay in the padding of a mirror's last tile (swap_remove re-tiles the removed last
row's tile to clear them).  Every filter kernel drops rows at or past n itself (k_gemm.hip, k_gemm8.hip, k_mfma.hip: `row < n`) and every
path that grows a mirror rewrites its ragged tile first, so stale padding changes no answer and no key of a row; no search can tell.

Wall time on one MI355X: 6 s for the 26 cases of this file (the longest, the first sequence A, 2 s with the library's first-use set-up;
every other case below 0.4 s); tests/test_edit_model_cpu.py: 6 s on the host.
"""
import numpy as np
import pytest

import edit_model as em

pytestmark = pytest.mark.gpu

DIM, N_BIG, N_SMALL, NQ, K = 128, 22037, 1003, 48, em.K
BIG = 5  # the row with the largest norm by far: never removed, moved or updated, so a patched and a fresh index share one fp16 scale
TIERS = {"i8": (2, 0), "fp16": (1, 2), "bf16": (1, 1)}  # flat_i8, flat_half  (with set_flat_mode(2))
DISTS = (("l2sqr", 0), ("cosine", 1))
COUNTERS = ("flat_i8_queries", "flat_half_queries")


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    return vdb


class Run:
    """one index and its model, written together"""

    def __init__(self, vdb, dist, kind, n, dim=DIM, u8=False, scale=1.0, seed=0, big=False, write_i8=None):
        self.vdb, self.dist, self.write_i8 = vdb, dist, write_i8
        off = np.random.default_rng([seed, 77]).standard_normal(dim) * 0.5
        self.model = em.EditModel(dim, kind, u8=u8, scale=scale, offset=None if u8 else off, seed=seed)
        first = self.model.vectors(n, 0)
        if big:
            first[BIG] *= 4
        self.ix = vdb.GpuIndex(dim, dist, scalar="u8" if u8 else "f32")
        self.rng = np.random.default_rng([seed, 78])
        self.pending = em.Touch()
        self.write(("add", first), note=f"{dist} dim {dim} scale {scale} seed {seed}: add <{n} rows>")

    def write(self, op, note=None):
        if self.write_i8 is not None:
            self.ix.set_param("flat_i8", self.write_i8)  # (the checks force tiers through this parameter: back to the sequence's own)
        em.apply_to_index(self.ix, op)
        t = self.model.apply(op, note)
        n, p = len(self.model), self.pending
        old = [v for v in (p.old_vecs, t.old_vecs) if v is not None and len(v)]
        self.pending = em.Touch(np.concatenate([p.new_at[p.new_at < n], t.new_at]), np.concatenate(old) if old else None,
                                np.concatenate([p.moved_to[p.moved_to < n], t.moved_to]))
        assert len(self.ix) == n, self.model.log
        return t

    def step(self, step):
        return self.write(self.model.expand(step), note=repr(step))

    def queries(self, nq=NQ):
        qs, hit = self.model.queries(self.rng, self.pending, nq)
        self.pending = em.Touch()
        return qs

    def force(self, tier):
        self.ix.set_flat_mode(2 if tier else 0)
        i8, half = TIERS[tier] if tier else (0, 0)
        self.ix.set_param("flat_i8", i8)
        self.ix.set_param("flat_half", half)

    def stats(self, *names):
        return [self.ix.get_stat(s) for s in names]

    def check(self, tier, qs=None, what=""):
        """k-NN of the aimed queries on a forced tier (None: nothing forced) == the oracle's, and the tier answered"""
        qs = self.queries() if qs is None else qs
        self.force(tier)
        i0, h0 = self.stats(*COUNTERS)
        em.check_knn(self.ix, self.model, qs, K, what=(what, tier))
        i1, h1 = self.stats(*COUNTERS)
        if tier == "i8":
            assert i1 >= i0 + len(qs) and self.stats("flat_i8_valid") == [1], (what, tier, i0, i1, self.model.log)
        elif tier == "fp16":
            assert h1 >= h0 + len(qs) and i1 == i0 and self.stats("flat_half_valid") == [1], (what, tier, h0, h1, self.model.log)
        elif tier == "bf16":
            assert (i1, h1) == (i0, h0) and self.stats("flat_bf16_mirror") == [1], (what, tier, self.model.log)
        return qs

    def close(self):
        self.ix.close()


def _fresh(vdb, run, prepared=True):
    ix = vdb.GpuIndex(run.model.dim, run.dist, scalar="u8" if run.model.u8 else "f32")
    em.apply_to_index(ix, ("add", run.model.rows))
    if prepared:
        ix.set_param("flat_i8", 1)
        ix.prepare(all_tiers=True)
        assert ix.get_stat("flat_half_valid") == 1 and ix.get_stat("flat_bf16_mirror") == 1
    return ix


# ---- A: shrink, then grow past the old extent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,kind", DISTS)
@pytest.mark.parametrize("tier", list(TIERS))
def test_a_shrink_then_grow_past_the_old_extent(vdb, tier, dist, kind):
    """Reached and asserted: split-bf16 mirror cut back by mirrors_shrunk and extended from its ragged tile (flat_bf16_mirror == 1
    throughout); fp16 mirror patched by the removes and the update, extended by the adds (flat_half_valid == 1 on the fp16 / bf16 runs; on
    the 8-bit run it is deferred, falls behind at the first add and is rebuilt for the key dump: test B pins that drop); 8-bit mirror
    patched by every remove / update that finds it in step (flat_i8_valid == 1), extended after a shrink with the old centre, and rebuilt
    once the table has twice the rows of its last re-centring.  At the end every forced search and the tier 0 / 1 keys equal a fresh index."""
    r = Run(vdb, dist, kind, N_BIG, seed=11, big=True)
    ix, m = r.ix, r.model
    ix.set_param("flat_i8", 1)
    ix.prepare(all_tiers=True)
    assert r.stats("flat_half_valid", "flat_bf16_mirror") == [1, 1]
    r.check(tier, what="A1")
    in_step = ["flat_i8_valid"] if tier == "i8" else ["flat_half_valid"]  # (8-bit run: the fp16 mirror is deferred, it falls behind at the first add)
    in_step.append("flat_bf16_mirror")
    # 2. a block of 2001 rows across the new end n' = 20036 = 16 * 1252 + 4
    t = r.write(("remove_rows", np.arange(19036, 21037)))
    moved = t.moved_to
    assert len(m) == 20036 and len(moved) == 1000 and r.stats("flat_half_valid", *in_step) == [1, 1, 1]
    r.check(tier, what="A2")
    # 3. more rows than were removed, the first an exact copy of a surviving row
    r.step(("add", 2600, 3, 77))
    assert len(m) == 22636 > N_BIG and r.stats("flat_bf16_mirror") == [1]
    qs = r.check(tier, what="A3")
    got = ix.flat_knn(m.rows[77:78], 2)
    assert got[0][0].tolist() == [77, 20036] and got[1][0, 0] == got[1][0, 1], "the tie between a row and its copy: the lower id first"
    # 4. swap_remove inside the last tile, of the last row, and of a row of tile 0 (the removed last row's tile is another one)
    for i in (22631, 22634, 3):  # of 22 636, 22 635 and 22 634 rows
        r.write(("swap_remove", i))
    assert len(m) == 22633 and r.stats(*in_step) == [1, 1]
    r.check(tier, what="A4")
    # 5. update: rows added in step 3, rows moved in step 2, the first tile (never row BIG); new vectors at half the scale
    ids = np.unique(np.concatenate([np.arange(20036, 20100), np.arange(22600, len(m)), moved[::25], [0, 1, 14, 15]]))
    ids = np.random.default_rng(12).permutation(ids)
    r.write(("update_rows", ids, (0.5 * m.vectors(len(ids), 5)).astype(np.float32)))
    assert r.stats(*in_step) == [1, 1]
    r.check(tier, what="A5")
    # 6. a random 60 % (row BIG stays where it is)
    pick = np.random.default_rng(13).permutation(len(m))[: len(m) * 6 // 10]
    r.write(("remove_rows", pick[pick != BIG]))
    assert r.stats(*in_step) == [1, 1]
    r.check(tier, what="A6")
    # 7. one row
    r.step(("add", 1, 7, -1))
    r.check(tier, what="A7")
    # 8. to more than twice the rows of the 8-bit mirror's last re-centring (step 1: 22 037 rows)
    r.step(("add", 2 * N_BIG + 17 - len(m), 8, 9))
    assert len(m) == 2 * N_BIG + 17 and r.stats("flat_bf16_mirror") == [1]
    qs = r.check(tier, what="A8")
    # a fresh index of the same rows, prepared the same way
    assert int(np.argmax((m.rows.astype(np.float64) ** 2).sum(1))) == BIG
    fresh = _fresh(vdb, r)
    r.force(tier)
    fresh.set_flat_mode(2)
    fresh.set_param("flat_i8", TIERS[tier][0])
    fresh.set_param("flat_half", TIERS[tier][1])
    a, b = ix.flat_knn(qs, K), fresh.flat_knn(qs, K)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), m.log
    for t in (0, 1):
        kp, kf = ix.flat_shortlist_keys(qs[:6], t), fresh.flat_shortlist_keys(qs[:6], t)
        assert kp[3]["xsq_max"] == kf[3]["xsq_max"] and kp[0].shape == kf[0].shape == (6, len(m)), (t, m.log)
        bad = np.flatnonzero((kp[0].view(np.uint32) != kf[0].view(np.uint32)).any(0))
        assert len(bad) == 0, ("tier", t, "keys differ at rows", bad[:8].tolist(), m.log)
    fresh.close()
    r.close()


# ---- B: the mirrors behind the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("write_i8", [0, 1], ids=["half_deferred", "half_extended"])
def test_b_mirrors_behind_the_table(vdb, write_i8):
    """flat_i8 = 0 while writing (the 8-bit tier is on, the fp16 mirror deferred): after an add both are behind, the update drops both
    (flat_i8_valid == 0, flat_half_valid == 0) and each is rebuilt in full by its next search.  flat_i8 = 1 (8-bit tier off): the add extends
    the fp16 mirror and the update patches it (flat_half_valid == 1).  The split-bf16 mirror is extended and patched in both (== 1)."""
    r = Run(vdb, "l2sqr", 0, N_BIG, seed=21, write_i8=write_i8)
    m = r.model
    qs = r.queries()
    for tier in TIERS:  # 1. every mirror exists and is in step
        r.check(tier, qs, what="B1")
    assert r.stats("flat_i8_valid", "flat_half_valid", "flat_bf16_mirror") == [1, 1, 1]
    r.step(("add", 33, 2, -1))  # 2. no search
    ids = np.array([N_BIG + 5, 3, 501, 500, N_BIG - 1, N_BIG + 32, 15])
    r.write(("update_rows", ids, m.vectors(len(ids), 3)))  # 3.
    assert r.stats("flat_i8_valid", "flat_half_valid", "flat_bf16_mirror") == [0, 1 if write_i8 else 0, 1], m.log
    qs = r.queries()
    for tier in TIERS:
        r.check(tier, qs, what="B3")
    r.step(("add", 700, 4, 100))  # 4. add, then remove across the new end, no search between them
    r.write(("remove_rows", np.concatenate([np.arange(N_BIG - 300, N_BIG + 200), [0, 17, 9000]])))
    assert r.stats("flat_i8_valid", "flat_half_valid", "flat_bf16_mirror") == [0, 1 if write_i8 else 0, 1], m.log
    qs = r.queries()
    for tier in TIERS:
        r.check(tier, qs, what="B4")
    r.force("i8")
    em.check_range(r.ix, m, qs, K, what="B4 range")
    r.close()


# ---- C: the fp16 scale ----------------------------------------------------------------------------------------------------------------------
def test_c_stale_fp16_scale_costs_margin_not_answers(vdb):
    """One row grows to 8 x the largest norm: the fp16 mirror is dropped (flat_half_valid == 0) and rebuilt with a larger exponent.  The row
    is removed: xsq_max and the exponent stay, as upper bounds.  An update of 10 % of the rows and an add then patch / extend the mirror
    under that stale scale (flat_half_valid == 1 after each): the answers stay the oracle's, and the mirror's scale stays the stale one."""
    r = Run(vdb, "l2sqr", 0, N_BIG, seed=31)
    ix, m = r.ix, r.model
    r.check("fp16", what="C0")
    big = int(np.argmax((m.rows.astype(np.float64) ** 2).sum(1)))
    r.write(("update_rows", np.array([5000]), (m.rows[big] * 8).reshape(1, -1)))
    assert r.stats("flat_half_valid") == [0]
    r.check("fp16", what="C1")
    xsq = ix.flat_shortlist_keys(m.rows[:1], 0)[3]["xsq_max"]
    assert xsq > 60 * (m.rows[big].astype(np.float64) ** 2).sum()  # (8 x the norm: 64 x its square)
    r.write(("remove_rows", np.array([5000])))
    assert r.stats("flat_half_valid") == [1]
    r.check("fp16", what="C2")
    r.step(("update_rows", N_BIG // 10, 4))
    assert r.stats("flat_half_valid") == [1]
    r.check("fp16", what="C3")
    r.step(("add", 211, 5, 40))
    assert r.stats("flat_half_valid") == [1]
    r.check("fp16", what="C4")
    assert ix.flat_shortlist_keys(m.rows[:1], 0)[3]["xsq_max"] == xsq  # still the removed row's
    em.check_rows(ix, m, np.arange(len(m)))
    r.close()


# ---- D: the gathered-row images under the IVF scan ------------------------------------------------------------------------------------------
def _ivf_pass(vdb, r, what):
    """ivf_build on the current rows, then (ivf_q8, ivf_half) in the four settings against oracle.IVF on the exported centroids and
    assignment, with the tier statistics of test_large_rows_gpu.py"""
    from oracle import oracle as O

    ix, m = r.ix, r.model
    ix.ivf_build(30, train_n=2000, max_iter=5, seed=3)
    ex = ix.ivf_export()
    iv = O.IVF(m.rows, ex["centroids"], m.kind, assign=ex["assign"])
    qs = r.queries(24)
    k, npb = 3, 30
    exp = [iv.knn(qs[q], k, npb) for q in range(len(qs))]
    try:
        for q8, half in ((2, 1), (1, 1), (0, 1), (1, 0)):
            ix.set_param("ivf_q8", q8)
            ix.set_param("ivf_half", half)
            idx, d, cnt = ix.ivf_knn(qs, k, npb)
            for q, (oi, od) in enumerate(exp):
                assert int(cnt[q]) == len(oi) == k and idx[q].tolist() == oi.tolist(), (what, q8, half, q, idx[q], oi, m.log)
                assert np.array_equal(d[q].view(np.uint32), od.view(np.uint32)), (what, q8, half, q, m.log)
            offers, kept, kept_q8 = r.stats("ivf_last_offers", "ivf_last_kept", "ivf_last_kept_q8")
            seen = (what, q8, half, offers, kept, kept_q8)
            assert (kept_q8 > 0) == (q8 != 0 and half != 0), seen
            if half:  # the fp16 tier answered: it passed on only part of the offers to the exact stage
                assert 0 < kept < offers, seen
            else:  # the plain scan: every offer reaches the exact stage
                assert kept == offers > 0, seen
    finally:
        ix.set_param("ivf_q8", 1)
        ix.set_param("ivf_half", 1)
    ix.ivf_clear()


def test_d_gathered_row_images_after_edits(vdb):
    """24 000 x 128, 30 clusters, (k, n_probes) = (3, 30): lists of 24 000 offers, far past 4 x max(1024, 64 k), so the 8-bit and the fp16
    pre-pass both run (ivf_last_kept_q8 > 0, 0 < ivf_last_kept < ivf_last_offers).  Both row-major images exist after the first pass; then
    an update alone (images dropped), an add alone (images EXTENDED from their old row count), remove + an update that outgrows the
    fp16 scale + add, and an add that outgrows the scale again (the fp16 image is rebuilt from row 0 under the new scale), each followed by a scan whose queries sit at the edited rows."""
    r = Run(vdb, "l2sqr", 0, 24000, seed=41)
    m = r.model
    r.ix.prof_enable(True)  # (the scan's tier statistics are kept by measurement calls)
    _ivf_pass(vdb, r, "D1")
    r.step(("update_rows", 300, 2))
    _ivf_pass(vdb, r, "D2 update")
    r.step(("add", 1500, 3, 10))
    _ivf_pass(vdb, r, "D3 add")
    r.write(("remove_rows", np.concatenate([np.arange(23000, 25000), np.arange(100, 3100, 3)])))
    big = int(np.argmax((m.rows.astype(np.float64) ** 2).sum(1)))
    ids = np.array([7, len(m) - 1, 12000])
    vecs = m.vectors(3, 4)
    vecs[2] = m.rows[big] * 8  # outgrows the fp16 scale
    r.write(("update_rows", ids, vecs))
    r.step(("add", 900, 5, -1))
    _ivf_pass(vdb, r, "D4 remove + update + add")
    vecs = m.vectors(40, 6)
    vecs[17] = m.rows[12000] * 8  # an add that outgrows the scale: the images cover the table, yet must be rebuilt from row 0
    r.write(("add", vecs))
    _ivf_pass(vdb, r, "D5 add past the scale")
    r.close()


# ---- E: labels and masks through shrink and grow -----------------------------------------------------------------------------------------
def _mask_words(allow):
    words = np.zeros((len(allow) + 63) // 64, dtype=np.uint64)
    ids = np.flatnonzero(allow)
    np.bitwise_or.at(words, ids // 64, np.uint64(1) << (ids % 64).astype(np.uint64))
    return words, ids.astype(np.uint32)


def _masks(r, terms_list):
    out = []
    for terms in terms_list:
        mk, allow = r.ix.make_mask_where(terms), r.model.where(terms)
        words, ids = mk.rows()
        ew, ei = _mask_words(allow)
        assert len(mk) == int(allow.sum()) and np.array_equal(words, ew) and np.array_equal(ids, ei), (terms, r.model.log)
        out.append((mk, allow))
    return out


def _masked_checks(r, masks, qs, big, what):
    ix, m = r.ix, r.model
    f0 = ix.get_stat("flat_filtered_i8_queries")
    for mk, allow in masks:
        em.check_filtered(ix, m, qs, mk, allow, K, what=what)
        em.check_range(ix, m, qs, K, mask=mk, allow=allow, what=what)
        codes = list(range(em.CODES)) + [em.NONE]
        for c in em.COLUMNS:
            assert np.array_equal(ix.label_counts(c, codes, mk), m.label_counts(c, codes, allow)), (what, c, m.log)
    if big:
        assert ix.get_stat("flat_filtered_i8_queries") >= f0 + len(masks) * len(qs), (what, m.log)


@pytest.mark.parametrize("n", [N_BIG, N_SMALL], ids=["i8_tier", "small_table"])
def test_e_labels_and_masks_through_shrink_and_grow(vdb, n):
    big = n == N_BIG
    r = Run(vdb, "l2sqr", 0, n, seed=51)
    ix, m = r.ix, r.model
    if big:
        r.force("i8")
        ix.set_param("flat_filtered_direct_max", 0)  # every allow-list takes the 8-bit filter pass with the masked row constants
    TERMS = ([(0, 1)], [(0, 2), (3, 0)], [(3, 1)])
    # 1. two columns, every row labelled in column 0, 90 % in column 3
    codes = em._codes(1, n)
    codes[codes == em.NONE] = 4  # (column 0 in full: an unlabelled row there must come from an add)
    r.write(("set_labels", 0, codes, 0))
    r.step(("set_labels", 3, 0, n, 2))
    old = _masks(r, TERMS)
    qs = r.queries()
    _masked_checks(r, old[:1], qs, big, "E1")
    # 2. / 3. remove: the labels moved with their rows, the old masks are refused
    r.write(("remove_rows", np.concatenate([np.arange(n - n // 5, n - n // 10), np.arange(3, n // 2, 7)])))
    em.check_labels(ix, m, "E3")
    for call in (lambda: ix.flat_knn_filtered(qs, K, old[0][0]), lambda: ix.range_search(qs, 1.0, mask=old[1][0]),
                 lambda: ix.flat_knn_filtered(qs, K, old[2][0])):
        with pytest.raises(vdb.VdbError, match="error 3"):  # VDB_ERR_STATE
            call()
    # 4. grow past the old extent: the new rows are unlabelled, also where labelled rows stood before the shrink
    n1 = len(m)
    r.step(("add", n - n1 + 37, 3, -1))
    for c in em.COLUMNS:
        got = ix.get_labels(c)
        assert (got[n1:] == em.NONE).all() and np.array_equal(got, m.labels[c]), ("E4", c, np.flatnonzero(got != m.labels[c])[:8], m.log)
    stale = ix.make_mask_where(TERMS[0])
    r.step(("add", 1, 4, -1))
    with pytest.raises(vdb.VdbError, match="error 3"):  # made before an add
        ix.flat_knn_filtered(qs, K, stale)
    # 5. scattered label writes on new and on moved rows
    ids = np.concatenate([np.arange(n1, len(m), 3), np.arange(3, n // 2, 7)[::2]])
    r.write(("set_labels_rows", ids, em.COLUMNS, np.stack([ids % 3, (ids // 3) % 2]).astype(np.uint32)))
    em.check_labels(ix, m, "E5")
    # 6. / 7. new masks == numpy, and the searches under them == the model
    new = _masks(r, TERMS)
    assert all(a.sum() >= K + 5 for _, a in new)
    qs = r.queries()
    _masked_checks(r, new, qs, big, "E7")
    # 8. update: the masks of step 6 stay valid, their row constants are rebuilt
    r.step(("update_rows", n // 10, 8))
    for lab in ((0, 2), (3, 1)):
        r.step(("set_labels_rows", 50, lab[:1], 9))  # (a label write does not stale a mask either: it keeps the rows it was built with)
    qs = r.queries()
    _masked_checks(r, new, qs, big, "E8")
    r.check("i8" if big else None, qs, what="E8 unfiltered")
    for mk, _ in old + new + [(stale, None)]:
        mk.close()
    r.close()


# ---- F: a u8 index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["fp16", "bf16"])
@pytest.mark.parametrize("dist,kind", DISTS)
def test_f_u8_index(vdb, tier, dist, kind):
    """u8 rows re-tile through widened chunks (for_tile_chunks) on every path: flat_half_queries rises and flat_half_valid stays 1 on the fp16 run,
    flat_bf16_mirror stays 1 on the split-bf16 run; the rows read back as stored; update_rows is refused and changes nothing"""
    from oracle import oracle as O

    r = Run(vdb, dist, kind, N_BIG, u8=True, seed=61)
    ix, m = r.ix, r.model
    r.check(tier, what="F0")
    mirror = "flat_half_valid" if tier == "fp16" else "flat_bf16_mirror"  # (the fp16 run never needs the split-bf16 mirror)
    r.write(("swap_remove", 20003))
    r.write(("swap_remove", len(m) - 1))
    r.check(tier, what="F1 swap_remove")
    r.write(("remove_rows", np.arange(19034, 21035)))  # across n' = 20034
    assert r.stats(mirror) == [1]  # patched through the widened chunks, not dropped
    r.check(tier, what="F2 remove_rows")
    r.step(("add", 2600, 3, 77))
    assert len(m) > N_BIG
    r.check(tier, what="F3 add")
    r.step(("remove_rows", "share", len(m) // 2, 4))
    r.step(("add", 1, 5, -1))
    qs = r.check(tier, what="F4 remove_rows + add")
    assert np.array_equal(ix.get_rows_u8(np.arange(len(m))), m.rows)
    idx, d, _ = ix.flat_knn_u8(qs[:6], 1)
    for q in range(6):  # the oracle's u8 fold itself
        assert np.float32(O.dist_u8(kind, m.rows[int(idx[q, 0])], qs[q])) == d[q, 0]
    with pytest.raises(vdb.VdbError, match="f32 rows"):
        ix.update_rows([1], np.zeros((1, DIM), dtype=np.float32))
    assert ix.get_stat("update_calls") == 0 and r.stats(mirror) == [1]
    em.check_rows(ix, m, np.arange(len(m)))
    r.check(tier, qs, what="F5 after the refusal")
    r.close()


# ---- the small-table paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,kind", DISTS)
def test_small_table_sequence(vdb, dist, kind):
    """1003 rows, nothing forced: 48 queries take the many-queries scan, 8 the one-launch kernel; both read the rows and norms themselves"""
    r = Run(vdb, dist, kind, N_SMALL, seed=71)
    m = r.model
    steps = [("remove_rows", "block", 850, 100), ("add", 300, 2, 40), ("swap_remove", 1199), ("swap_remove", 1201), ("swap_remove", 2),
             ("update_rows", 120, 3), ("remove_rows", "share", 720, 4), ("add", 1, 5, -1), ("remove_rows", "last_tile"), ("add", 40, 6, 0)]
    for st in steps:
        r.step(st)
        if st[0] == "swap_remove" and st[1] != 2:
            continue
        qs = r.check(None, what=st)
        r.check(None, qs[:8], what=(st, "8 queries"))
        em.check_range(r.ix, m, qs, K, what=st)
    em.check_rows(r.ix, m, np.arange(len(m)))
    r.close()


# ---- seeded random sequences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_random_sequence(vdb, seed):
    rng = np.random.default_rng([1806, seed])
    dim = (64, 128, 192)[seed % 3]
    dist, kind = DISTS[(seed // 3) % 2]
    scale = (0.05, 1.0, 30.0)[(seed + seed // 3) % 3]
    n0 = (3011, 9005, 17003)[(seed + seed // 4) % 3]
    r = Run(vdb, dist, kind, n0, dim=dim, scale=scale, seed=100 + seed)
    ix, m = r.ix, r.model
    tiers = ["bf16", None] if dim == 64 else ["i8", "fp16", "bf16", None]
    steps = em.draw_steps(rng, m, int(rng.integers(10, 15)), min_rows=300)
    m.log.append(f"steps = {steps!r}")
    for st in steps:
        t = r.step(st)
        check = ("knn", "filtered", "range", "rows")[int(rng.integers(4))]
        tier = tiers[int(rng.integers(len(tiers)))]
        what = (st, check, tier)
        if check == "knn":
            r.check(tier, what=what)
        elif check == "rows":
            em.check_rows(ix, m, np.unique(np.concatenate([t.new_at, t.moved_to, [0, len(m) - 1]])), what=what)
            em.check_labels(ix, m, what=what)
        else:
            r.force(tier)
            qs = r.queries()
            if check == "range":
                em.check_range(ix, m, qs, K, what=what)
            else:
                allow = rng.random(len(m)) < (0.5, 0.9, 0.02)[int(rng.integers(3))]
                if 0 in m.labels and (m.labels[0] == 1).sum() >= 64 and rng.random() < 0.5:
                    mk, allow = ix.make_mask_where([(0, 1)]), m.where([(0, 1)])
                else:
                    allow[:64] = True
                    mk = ix.make_mask(allow)
                em.check_filtered(ix, m, qs, mk, allow, K, what=what)
                mk.close()
    r.check(tiers[0], what="end")
    em.check_rows(ix, m, np.arange(len(m)), what="end")
    em.check_labels(ix, m, what="end")
    r.close()
