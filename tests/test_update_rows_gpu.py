"""GPU: in-place row update (vdb_index_update_rows / GpuIndex.update_rows; csrc/k_update.hip and the tile-list forms of the re-tiling kernels).

After the call every search must answer exactly as the oracle does on the table with those rows replaced.  Checked: (1) the rows
themselves, bit for bit against the numpy-updated table; (2) searches on every Flat tier right after the call, with queries at the NEW
and at the OLD vectors of updated rows (a stale tile would return the old row at distance ~ 0); (3) the fp16 / split-bf16 mirrors' keys
against a FRESH index built from the updated table; (4) an update that outgrows the fp16 scale; (5) NaN / inf / zero / duplicate rows;
(6) a mirror that was behind the table; (7) masks made before the call stay valid and their row-constant copies are rebuilt; (8) labels;
(9) the device form; (10) refusals.  Shapes: 22 037 rows x 128 is the smallest the forced tiers take, ragged against 16 and 192; 1003 rows
for the small-table paths.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 128
N_BIG, N_SMALL = 22037, 1003
TIERS = {"i8": (2, 0), "fp16": (1, 2), "bf16": (1, 1)}  # flat_i8, flat_half  (with set_flat_mode(2))
DISTS = (("l2sqr", 0), ("cosine", 1))
MASK_STATS = ("mask_where_masks", "mask_where_set_masks", "mask_where_any_masks", "mask_combine_masks", "mask_partition_masks")


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


def _gauss(rng, n, off):
    return (rng.standard_normal((n, DIM)) + off).astype(np.float32)


def _sets(n, rng):
    last0 = n - n % 16  # first row of the ragged last tile
    assert n % 16 >= 3 and n % 192
    return {
        "random10": rng.permutation(n)[: n // 10],
        "first_tile": np.arange(1, 14),
        "last_tile": np.arange(last0 + 1, n),
        "block_over_unit": np.arange(192 * 3 - 40, 192 * 3 + 40),  # contiguous, across a 192-row unit boundary
        "one": np.array([n // 2]),
        "all": np.arange(n),
    }


def _index(vdb, dist, base, tier=None):
    ix = vdb.GpuIndex(DIM, dist)
    ix.batch_add(base)
    if tier is not None:
        ix.set_flat_mode(2)
        ix.set_param("flat_i8", TIERS[tier][0])
        ix.set_param("flat_half", TIERS[tier][1])
    return ix


# ---- (1) the rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pattern", [(N_BIG, p) for p in ("random10", "first_tile", "last_tile", "block_over_unit", "one")] +
                         [(N_SMALL, p) for p in ("random10", "last_tile", "one", "all")])
def test_rows_equal_the_numpy_updated_table(mods, n, pattern):
    vdb, _ = mods
    rng = np.random.default_rng(31)
    off = rng.standard_normal(DIM) * 0.5
    base = _gauss(rng, n, off)
    rows = rng.permutation(_sets(n, rng)[pattern])  # ids are passed shuffled
    new = _gauss(rng, len(rows), off)
    after = base.copy()
    after[rows] = new
    ix = _index(vdb, "l2sqr", base)
    ix.set_flat_mode(2)
    ix.flat_knn(base[:2], 3)  # (a mirror is live, so that the tile rewrite runs under every pattern)
    ix.update_rows(rows, new)
    assert len(ix) == n
    assert ix.get_stat("update_calls") == 1 and ix.get_stat("update_rows") == len(rows)
    look = range(n) if n == N_SMALL else sorted(set(rows.tolist()) | set(range(0, n, 997)) | {n - 1})
    for i in look:
        assert np.array_equal(ix[i].view(np.uint32), after[i].view(np.uint32)), i
    ix.close()


# ---- (2) searches right after the call ------------------------------------------------------------------------------------------------
def _case(O, n, seed, kinds=(0, 1)):
    """base rows, the update (random 10 % + the first tile's rows + the ragged last tile's + a block across a unit boundary; ids shuffled),
    the updated table, 64 queries (32 at NEW vectors of updated rows, 32 at OLD vectors of updated rows, + 1e-3 noise) and per metric the
    oracle's top 12 on the updated table"""
    rng = np.random.default_rng(seed)
    off = rng.standard_normal(DIM) * 0.5
    base = _gauss(rng, n, off)
    s = _sets(n, rng)
    rows = np.unique(np.concatenate([s["random10"], s["first_tile"], s["last_tile"], s["block_over_unit"]]))
    rows = rng.permutation(rows)
    new = _gauss(rng, len(rows), off)
    after = base.copy()
    after[rows] = new
    pick_new = np.linspace(0, len(rows) - 1, 32).astype(int)
    pick_old = (pick_new + 7) % len(rows)
    qs = (np.concatenate([new[pick_new], base[rows[pick_old]]]) + 1e-3 * rng.standard_normal((64, DIM))).astype(np.float32)
    top = {kind: O.flat_knn_batch(after, qs, 12, kind, nthreads=8) for kind in kinds}
    for kind in kinds:  # the queries at new vectors find exactly that row
        assert top[kind][0][:32, 0].astype(np.int64).tolist() == rows[pick_new].tolist()
    return dict(base=base, rows=rows, new=new, after=after, qs=qs, top=top, off=off)


def _expect_range(top, k=7):
    oi, od, _ = top
    radius = od[:, k - 1].copy()
    lims, ids, ds = [0], [], []
    for q in range(len(oi)):
        cut = int((od[q] <= radius[q]).sum())
        assert k <= cut < od.shape[1]  # the 12 oracle rows hold the whole ball
        ids.append(oi[q, :cut])
        ds.append(od[q, :cut])
        lims.append(lims[-1] + cut)
    return radius, np.array(lims, dtype=np.uint64), np.concatenate(ids).astype(np.uint64), np.concatenate(ds)


def _check_searches(ix, case, kind, nq=64):
    oi, od, oc = (a[:nq] for a in case["top"][kind])
    idx, d, cnt = ix.flat_knn(case["qs"][:nq], 7)
    assert cnt.tolist() == [7] * nq
    assert np.array_equal(idx, oi[:, :7].astype(np.uint64)), np.nonzero((idx != oi[:, :7]).any(1))
    assert np.array_equal(d.view(np.uint32), od[:, :7].view(np.uint32))
    radius, el, ei, ed = _expect_range((oi, od, oc))
    gl, gi, gd = ix.range_search(case["qs"][:nq], radius)
    assert np.array_equal(gl, el) and np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32))


@pytest.fixture(scope="module")
def big_case(mods):
    return _case(mods[1], N_BIG, 32)


@pytest.fixture(scope="module")
def small_case(mods):
    return _case(mods[1], N_SMALL, 33)


@pytest.mark.parametrize("dist,kind", DISTS)
@pytest.mark.parametrize("tier", ["i8", "fp16", "bf16"])
def test_search_after_update_per_tier(mods, big_case, tier, dist, kind):
    vdb, _ = mods
    c = big_case
    ix = _index(vdb, dist, c["base"], tier)
    ix.flat_knn(c["qs"], 7)  # the tier's mirror is built and in step with the table
    if tier == "i8":
        assert ix.get_stat("flat_i8_valid") == 1
    before = {s: ix.get_stat(s) for s in ("flat_i8_queries", "flat_half_queries")}
    ix.update_rows(c["rows"], c["new"])
    assert len(ix) == N_BIG
    if tier == "i8":
        assert ix.get_stat("flat_i8_valid") == 1  # kept, not dropped for a rebuild
    _check_searches(ix, c, kind)
    if tier == "i8":
        assert ix.get_stat("flat_i8_valid") == 1 and ix.get_stat("flat_i8_queries") >= before["flat_i8_queries"] + 64
    if tier == "fp16":
        assert ix.get_stat("flat_half_queries") >= before["flat_half_queries"] + 64
    ix.close()


@pytest.mark.parametrize("dist,kind", DISTS)
def test_search_after_update_small_table(mods, small_case, dist, kind):
    """1003 rows, nothing forced: the one-launch kernel / the scan read the rows and the norms themselves"""
    vdb, _ = mods
    c = small_case
    ix = _index(vdb, dist, c["base"])
    ix.flat_knn(c["qs"][:4], 7)
    ix.update_rows(c["rows"], c["new"])
    _check_searches(ix, c, kind)
    _check_searches(ix, c, kind, nq=8)  # (fewer than 32 queries: k_flat_small)
    ix.close()


# ---- (3) mirror keys against a fresh index ----------------------------------------------------------------------------------------------
def _prepared(vdb, rows):
    ix = vdb.GpuIndex(DIM, "l2sqr")
    ix.batch_add(rows)
    ix.set_param("flat_i8", 1)
    ix.prepare(all_tiers=True)
    assert ix.get_stat("flat_half_valid") == 1 and ix.get_stat("flat_bf16_mirror") == 1
    return ix


def test_mirror_keys_equal_a_fresh_index(mods, big_case):
    """fp16 (tier 0) and split-bf16 (tier 1) keys of every row: the updated index == an index built from the updated table, bit for bit;
    one call == two calls of shuffled halves.  Row 0 carries the largest norm by far and is never updated, so both have one fp16 scale."""
    vdb, _ = mods
    c = big_case
    keep = c["rows"] != 0
    rows, new = c["rows"][keep], c["new"][keep]
    base, after = c["base"].copy(), c["after"].copy()
    base[0] *= 4
    after[0] = base[0]
    ix, fresh, halves = _prepared(vdb, base), _prepared(vdb, after), _prepared(vdb, base)
    ix.update_rows(rows, new)
    perm = np.random.default_rng(34).permutation(len(rows))
    a, b = perm[: len(perm) // 2], perm[len(perm) // 2:]
    halves.update_rows(rows[a], new[a])
    halves.update_rows(rows[b], new[b])
    for x in (ix, halves):
        assert x.get_stat("flat_half_valid") == 1 and x.get_stat("flat_bf16_mirror") == 1  # kept in step, not dropped
    qs = c["qs"][28:36]  # at new and at old vectors
    for tier in (0, 1):
        ku, kf, kh = (x.flat_shortlist_keys(qs, tier) for x in (ix, fresh, halves))
        assert ku[0].shape == (8, N_BIG)
        assert np.array_equal(ku[0].view(np.uint32), kf[0].view(np.uint32)), tier
        assert np.array_equal(ku[0].view(np.uint32), kh[0].view(np.uint32)), tier
        assert ku[3]["xsq_max"] == kf[3]["xsq_max"]
        assert ku[3]["dx_abs"] >= kf[3]["dx_abs"] and ku[3]["dx_rel"] >= kf[3]["dx_rel"]  # bounds: folded in, never narrowed
        assert ku[3] == kh[3]
    for x in (ix, fresh, halves):
        x.close()


# ---- (4) an update that outgrows the fp16 scale ---------------------------------------------------------------------------------------
def test_fp16_scale_outgrown(mods, big_case):
    vdb, O = mods
    c = big_case
    ix = _index(vdb, "l2sqr", c["base"], "fp16")
    ix.flat_knn(c["qs"], 7)
    assert ix.get_stat("flat_half_valid") == 1
    big = int(np.argmax((c["base"].astype(np.float64) ** 2).sum(1)))
    vec = (c["base"][big] * 64).astype(np.float32)  # 64 x the largest norm
    ix.update_rows([5000], vec.reshape(1, -1))
    assert ix.get_stat("flat_half_valid") == 0
    after = c["base"].copy()
    after[5000] = vec
    qs = np.concatenate([c["qs"][:15], (vec + 1e-3).reshape(1, -1)]).astype(np.float32)
    h0 = ix.get_stat("flat_half_queries")
    idx, d, cnt = ix.flat_knn(qs, 7)
    oi, od, oc = O.flat_knn_batch(after, qs, 7, 0, nthreads=8)
    assert np.array_equal(idx, oi.astype(np.uint64)) and np.array_equal(d.view(np.uint32), od.view(np.uint32))
    assert idx[15, 0] == 5000
    assert ix.get_stat("flat_half_valid") == 1 and ix.get_stat("flat_half_queries") >= h0 + 16
    ix.close()


# ---- (5) special rows -------------------------------------------------------------------------------------------------------------------
def _same_knn(got, exp, what=""):
    (gi, gd, gc), (ei, ed, ec) = got, exp
    assert np.array_equal(gc, ec), (what, gc, ec)
    assert np.array_equal(gi, ei.astype(np.uint64)), what
    assert gd.dtype == np.float32 and np.array_equal(np.isnan(gd), np.isnan(ed)), what  # (a NaN's payload is not part of the contract)
    ok = ~np.isnan(ed)
    assert np.array_equal(gd[ok].view(np.uint32), ed[ok].view(np.uint32)), what


@pytest.mark.parametrize("dist,kind", DISTS)
def test_special_rows(mods, small_case, dist, kind):
    """rows updated to a NaN element, an inf element, the zero vector and an exact duplicate of a lower-numbered row, on the 8-bit tier"""
    vdb, O = mods
    c = small_case
    base = c["base"]
    rng = np.random.default_rng(35)
    rows = np.array([900, 17, 333, 612])
    new = _gauss(rng, 4, c["off"])
    new[0, 17] = np.nan
    new[1, 100] = np.inf
    new[2] = 0.0
    new[3] = base[40]  # tie with row 40: the lower id first
    after = base.copy()
    after[rows] = new
    qs = np.concatenate([base[[40, 41, 900, 17]], new[2:3] + np.float32(0.5), _gauss(rng, 3, c["off"])]).astype(np.float32)
    ix = _index(vdb, dist, base, "i8")
    ix.flat_knn(qs, 3)
    assert ix.get_stat("flat_i8_valid") == 1
    ix.update_rows(rows, new)
    for k in (7, N_SMALL):  # (k = every row: the NaN distances last)
        exp = O.flat_knn_batch(after, qs, k, kind, nthreads=8)
        _same_knn(ix.flat_knn(qs, k), exp, (dist, k))
    got = ix.flat_knn(qs[:1], 2)
    assert got[0][0].tolist() == [40, 612]
    ix.close()


# ---- (6) a mirror behind the table ------------------------------------------------------------------------------------------------------
def test_mirror_behind_the_table(mods):
    """batch_add, then update_rows before any search: the 8-bit mirror is behind, dropped, and rebuilt by the next search"""
    vdb, O = mods
    rng = np.random.default_rng(36)
    n = 20005
    base = rng.standard_normal((n + 33, DIM)).astype(np.float32)
    ix = _index(vdb, "l2sqr", base[:n], "i8")
    ix.flat_knn(base[:5], 7)
    assert ix.get_stat("flat_i8_valid") == 1
    ix.batch_add(base[n:])
    rows = np.array([n + 5, 3, 501, 500, n - 1])
    new = rng.standard_normal((5, DIM)).astype(np.float32)
    ix.update_rows(rows, new)
    assert ix.get_stat("flat_i8_valid") == 0
    after = base.copy()
    after[rows] = new
    qs = (np.concatenate([new, base[[3, 500, n + 5, 19000]]]) + 1e-3 * rng.standard_normal((9, DIM))).astype(np.float32)
    idx, d, cnt = ix.flat_knn(qs, 7)
    oi, od, oc = O.flat_knn_batch(after, qs, 7, 0, nthreads=8)
    assert cnt.tolist() == oc.tolist() and np.array_equal(idx, oi.astype(np.uint64)) and np.array_equal(d, od)
    assert idx[:5, 0].tolist() == rows.tolist()
    assert ix.get_stat("flat_i8_valid") == 1
    ix.close()


# ---- (7) masks survive ------------------------------------------------------------------------------------------------------------------
def _restrict(full, allow, k):
    oi, od = full
    idx = np.zeros((len(oi), k), dtype=np.uint64)
    dist = np.zeros((len(oi), k), dtype=np.float32)
    for q in range(len(oi)):
        keep = allow[q][oi[q].astype(np.int64)] if isinstance(allow, list) else allow[oi[q].astype(np.int64)]
        idx[q], dist[q] = oi[q][keep][:k], od[q][keep][:k]
    return idx, dist


@pytest.mark.parametrize("dist,kind", DISTS)
def test_masks_made_before_the_update_stay_valid(mods, big_case, dist, kind):
    vdb, O = mods
    c = big_case
    n, k = N_BIG, 5
    base = c["base"]
    rng = np.random.default_rng(37)
    allow_long = np.arange(n) % 2 == 0  # 11 019 rows > flat_filtered_direct_max: the 8-bit tier
    allow_short = np.zeros(n, dtype=np.bool_)
    allow_short[rng.permutation(n)[:700]] = True  # the direct path
    ix = _index(vdb, dist, base)
    ix.set_flat_mode(2)
    mk_long, mk_short = ix.make_mask(allow_long), ix.make_mask(allow_short)
    assert len(mk_long) == 11019 > 8192 and len(mk_short) == 700
    f0 = ix.get_stat("flat_filtered_i8_queries")
    ix.flat_knn_filtered(base[:8], k, mk_long)  # the masked copy of the row constants exists now
    assert ix.get_stat("flat_filtered_i8_queries") == f0 + 8
    # updated rows: allowed and disallowed ones of both masks
    in_short, out_short = np.flatnonzero(allow_short), np.flatnonzero(~allow_short)
    rows = np.unique(np.concatenate([in_short[:40], out_short[:60], np.arange(3000, 3300), c["rows"][:500]]))
    rows = rng.permutation(rows)
    new = _gauss(rng, len(rows), c["off"])
    after = base.copy()
    after[rows] = new
    m0 = {s: ix.get_stat(s) for s in MASK_STATS}
    ix.update_rows(rows, new)
    # queries at the new vectors of updated rows: 4 allowed by the long mask, 4 not; 4 allowed by the short mask, 4 not
    upd_long = [np.flatnonzero(allow_long[rows] == a)[:4] for a in (True, False)]
    upd_short = [np.flatnonzero(allow_short[rows] == a)[:4] for a in (True, False)]
    pick = np.concatenate(upd_long + upd_short)
    qs = (new[pick] + 1e-3 * rng.standard_normal((16, DIM))).astype(np.float32)
    oi, od, oc = O.flat_knn_batch(after, qs, n, kind, nthreads=16)
    full = (oi.astype(np.uint64), od)
    f1 = ix.get_stat("flat_filtered_i8_queries")
    for mk, allow, hit, miss in ((mk_long, allow_long, range(0, 4), range(4, 8)), (mk_short, allow_short, range(8, 12), range(12, 16))):
        ei, ed = _restrict(full, allow, k)
        gi, gd, gc = ix.flat_knn_filtered(qs, k, mk)
        assert gc.tolist() == [k] * 16 and np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32))
        assert gi[list(hit), 0].tolist() == rows[pick[list(hit)]].tolist()  # updated allowed rows: found at rank 0
        assert not np.isin(rows[pick[list(miss)]], gi[list(miss)]).any()      # updated disallowed rows: absent
        lims, ri, rd = ix.range_search(qs, ed[:, k - 1], mask=mk)
        assert lims.tolist() == list(range(0, 16 * k + 1, k))  # (no ties among gaussian rows)
        assert np.array_equal(ri.reshape(16, k), ei) and np.array_equal(rd.reshape(16, k).view(np.uint32), ed.view(np.uint32))
    assert ix.get_stat("flat_filtered_i8_queries") >= f1 + 16  # the long mask took the 8-bit tier, with rebuilt row constants
    mask_of = [q % 2 for q in range(16)]
    ei, ed = _restrict(full, [(allow_long, allow_short)[m] for m in mask_of], k)
    gi, gd, gc = ix.flat_knn_filtered_multi(qs, k, [mk_long, mk_short], mask_of)
    assert np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32))
    assert {s: ix.get_stat(s) for s in MASK_STATS} == m0  # nothing rebuilt a mask
    ix.batch_add(base[:1])
    for call in (lambda: ix.flat_knn_filtered(qs, k, mk_long), lambda: ix.range_search(qs, 1.0, mask=mk_short),
                 lambda: ix.flat_knn_filtered_multi(qs, k, [mk_long, mk_short], mask_of)):
        with pytest.raises(vdb.VdbError, match="error 3"):  # VDB_ERR_STATE: rows were added, the masks ARE stale now
            call()
    mk_long.close()
    mk_short.close()
    ix.close()


# ---- (8) labels -------------------------------------------------------------------------------------------------------------------------
NONE = 0xFFFFFFFF


def _walk(codes, g, k):
    kept, seen = [], {}
    for p, c in enumerate(codes.tolist()):
        if len(kept) == k:
            break
        if c != NONE:
            if seen.get(c, 0) >= g:
                continue
            seen[c] = seen.get(c, 0) + 1
        kept.append(p)
    return kept


def test_labels_are_untouched(mods, small_case):
    vdb, O = mods
    c = small_case
    n = N_SMALL
    rng = np.random.default_rng(38)
    col0 = rng.integers(0, 6, n).astype(np.uint32)
    col3 = rng.integers(0, 40, n).astype(np.uint32)
    col3[rng.permutation(n)[:100]] = NONE
    ix, fresh = _index(vdb, "l2sqr", c["base"]), _index(vdb, "l2sqr", c["after"])
    for x in (ix, fresh):
        x.set_labels(0, col0)
        x.set_labels(3, col3)
    ix.update_rows(c["rows"], c["new"])
    qs = c["qs"][24:40]
    oi, od, oc = O.flat_knn_batch(c["after"], qs, n, 0, nthreads=8)
    for col, codes in ((0, col0), (3, col3)):
        assert np.array_equal(ix.get_labels(col), codes) and np.array_equal(fresh.get_labels(col), codes)
        want = list(range(int(codes[codes != NONE].max()) + 1)) + [NONE]
        assert np.array_equal(ix.label_counts(col, want), fresh.label_counts(col, want))
        assert ix.label_counts(col, want).tolist() == [int((codes == w).sum()) for w in want]
        gi, gd, gc = ix.flat_knn_grouped(qs, 6, col, 2)
        fi, fd, fc = fresh.flat_knn_grouped(qs, 6, col, 2)
        assert np.array_equal(gi, fi) and np.array_equal(gd.view(np.uint32), fd.view(np.uint32)) and np.array_equal(gc, fc)
        for q in range(len(qs)):
            kept = _walk(codes[oi[q].astype(np.int64)], 2, 6)
            assert gc[q] == len(kept) and gi[q, : len(kept)].tolist() == oi[q][kept].tolist()
            assert np.array_equal(gd[q, : len(kept)].view(np.uint32), od[q][kept].view(np.uint32))
    ix.close()
    fresh.close()


# ---- (9) the device form ----------------------------------------------------------------------------------------------------------------
def test_device_form(mods, big_case):
    import torch

    vdb, _ = mods
    c = big_case
    d_new = torch.from_numpy(c["new"]).cuda()
    torch.cuda.synchronize()
    for tier in TIERS:
        ix = _index(vdb, "l2sqr", c["base"], tier)
        ix.flat_knn(c["qs"], 7)
        ix.update_rows_device(c["rows"], d_new.data_ptr())
        assert len(ix) == N_BIG and ix.get_stat("update_rows") == len(c["rows"])
        _check_searches(ix, c, 0)
        for i in c["rows"][:50].tolist() + [0, N_BIG - 1]:
            assert np.array_equal(ix[i].view(np.uint32), c["after"][i].view(np.uint32)), i
        ix.close()


# ---- (10) refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_index_unchanged(mods):
    vdb, _ = mods
    rng = np.random.default_rng(39)
    n = 600
    base = rng.standard_normal((n, 32)).astype(np.float32)
    new = rng.standard_normal((2, 32)).astype(np.float32)
    ix = vdb.GpuIndex(32, "l2sqr")
    ix.batch_add(base)
    mk = ix.make_mask(np.arange(n) % 2 == 0)

    def unchanged():
        ok = len(ix) == n and np.array_equal(ix[0], base[0]) and np.array_equal(ix[n - 1], base[n - 1])
        ok = ok and ix.get_stat("update_calls") == 0 and ix.get_stat("update_rows") == 0
        idx, d, cnt = ix.flat_knn_filtered(base[[0, 2, 4]], 2, mk)  # the mask is still usable
        return ok and idx[:, 0].tolist() == [0, 2, 4]

    ix.pq_build(n_bits=4, m=8, train_n=200, max_iter=2)
    with pytest.raises(vdb.VdbError, match="update_rows invalidates the PQ table: clear it first"):
        ix.update_rows([0, n - 1], new)
    ix.pq_clear()
    assert unchanged()
    ix.hnsw_build(M=8, ef_construction=20)
    with pytest.raises(vdb.VdbError, match="update_rows needs a Flat index"):
        ix.update_rows([0, n - 1], new)
    ix.hnsw_clear()
    assert unchanged()
    ix.ivf_build(8, max_iter=2)
    with pytest.raises(vdb.VdbError, match="update_rows invalidates the IVF clusters: clear them first"):
        ix.update_rows([0, n - 1], new)
    ix.ivf_clear()
    assert unchanged()
    with pytest.raises(vdb.VdbError, match="error 1"):  # an id == n
        ix.update_rows([0, n], new)
    for bad_rows in ([4, 4], [-1, 3], [1.5, 2.0], [True, False]):
        with pytest.raises(ValueError):
            ix.update_rows(bad_rows, new)
    for bad_vecs in (new[:1], new[:, :31], new.ravel(), np.zeros((2, 33), dtype=np.float32)):  # not (len(rows), dim)
        with pytest.raises(vdb.VdbError, match="dimension mismatch"):
            ix.update_rows([0, n - 1], bad_vecs)
    from lab_1806_vec_db_amd import _lib as L
    dup = np.array([n - 1, 0, n - 1], dtype=np.uint64)  # a duplicate handed to the ABI itself
    three = np.zeros((3, 32), dtype=np.float32)
    assert ix._lib.vdb_index_update_rows(ix._h, dup.ctypes.data_as(L.u64p), 3, three.ctypes.data_as(L.f32p)) == 1
    assert b"duplicate" in ix._lib.vdb_last_error()
    assert unchanged()
    ix.update_rows([], np.zeros((0, 32), dtype=np.float32))  # m == 0: a no-op that counts nothing
    assert ix._lib.vdb_index_update_rows(ix._h, None, 0, None) == 0
    assert unchanged()
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.flat_knn(base[:3], 2)
    v0 = ix.get_stat("flat_i8_valid")
    with pytest.raises(vdb.VdbError, match="error 1"):
        ix.update_rows([0, n], new)
    assert ix.get_stat("flat_i8_valid") == v0 and unchanged()
    ix.update_rows([n - 1, 0], new)  # and the index still works
    assert np.array_equal(ix[0], new[1]) and np.array_equal(ix[n - 1], new[0]) and np.array_equal(ix[1], base[1])
    assert ix.get_stat("update_calls") == 1 and ix.get_stat("update_rows") == 2
    idx, d, cnt = ix.flat_knn_filtered(new[1:2], 1, mk)  # the mask made before all this still works, on the new row
    assert idx[0, 0] == 0 and d[0, 0] == 0.0
    mk.close()
    ix.close()
    u8 = vdb.GpuIndex(30, "l2sqr", scalar="u8")
    u8.batch_add_u8(rng.integers(0, 256, size=(50, 30), dtype=np.uint8))
    with pytest.raises(vdb.VdbError, match="f32 rows"):
        u8.update_rows([1], np.zeros((1, 30), dtype=np.float32))
    assert len(u8) == 50 and u8.get_stat("update_calls") == 0
    u8.close()
