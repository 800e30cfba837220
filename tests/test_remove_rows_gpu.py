"""GPU: bulk row removal (vdb_index_remove_rows / GpuIndex.remove_rows; csrc/k_remove.hip and the tile-list forms of the re-tiling kernels).

Removing the rows R must leave the state that swap_remove on them in DESCENDING order leaves.  Checked: (1) the rows themselves, bit for
bit against a twin index that runs that loop, for f32 rows and for a VecSet<u8> index whose 30-byte rows take the byte path of the move
kernel; (2) searches on every Flat tier right after the call, against the oracle on the numpy-replayed rows, with queries that make a
stale tile visible; (3) the fp16 / split-bf16 mirrors' keys against the twin's; (4) a mirror that was behind the table; (5) masks;
(6) refusals.  Shapes: 20 000 rows x 128 is the smallest the forced tiers take; n and n' are ragged (no multiple of 16 or of 192).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 128
TIERS = {"i8": (2, 0), "fp16": (1, 2), "bf16": (1, 1)}  # flat_i8, flat_half  (with set_flat_mode(2))


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


def _replay(n, rows):
    """original row ids, in table order, after swap_remove on `rows` in descending order"""
    cur = np.arange(n)
    last = n
    for i in sorted((int(r) for r in rows), reverse=True):
        last -= 1
        cur[i] = cur[last]
    return cur[:last]


def _patterns(n, rng):
    m10 = n // 10
    n1 = n - m10
    return {
        "random10": rng.permutation(n)[:m10],
        "random60": rng.permutation(n)[: (n * 6) // 10],  # n' < m: most of the tail is removed too
        "last_tile": np.arange(n - 9, n - 1),             # inside the ragged last tile: one hole below n', the rest in the tail
        "first_tile": np.arange(1, 14),
        "block_over_boundary": np.arange(n1 - m10 // 2, n1 - m10 // 2 + m10),  # contiguous, across n'
    }


def _rows_of(ix, u8):
    return np.stack([ix.row_u8(i) if u8 else ix[i] for i in range(len(ix))]) if len(ix) else np.zeros((0, ix.dim))


def _table(vdb, kind, n, rng):
    if kind == "u8":
        base = rng.integers(0, 256, size=(n, 30), dtype=np.uint8)
        ix, twin = vdb.GpuIndex(30, "l2sqr", scalar="u8"), vdb.GpuIndex(30, "l2sqr", scalar="u8")
        ix.batch_add_u8(base)
        twin.batch_add_u8(base)
    else:
        base = rng.standard_normal((n, DIM)).astype(np.float32)
        ix, twin = vdb.GpuIndex(DIM, "l2sqr"), vdb.GpuIndex(DIM, "l2sqr")
        ix.batch_add(base)
        twin.batch_add(base)
    return base, ix, twin


@pytest.mark.parametrize("pattern", ["random10", "random60", "last_tile", "first_tile", "block_over_boundary"])
@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_state_equals_the_swap_remove_loop(mods, kind, pattern):
    vdb, _ = mods
    rng = np.random.default_rng(11)
    n = 20011  # = 16 * 1250 + 11 = 192 * 104 + 43
    base, ix, twin = _table(vdb, kind, n, rng)
    rows = _patterns(n, rng)[pattern]
    n1 = n - len(rows)
    assert n1 % 16 and n1 % 192
    tiers = ((1, 2), (1, 1)) + (((2, 0),) if kind == "f32" else ())  # (flat_i8, flat_half): fp16, split-bf16, 8-bit
    ix.set_flat_mode(2)
    for i8, half in tiers:  # every mirror the shape has is live, so that the tile rewrites run under every pattern
        ix.set_param("flat_i8", i8)
        ix.set_param("flat_half", half)
        ix.flat_knn(base[:2].astype(np.float32), 3)
    # (30 columns pad to ONE 64-column block: the u8 table has the split-bf16 mirror only, the fp16 / 8-bit passes want two blocks)
    assert ix.get_stat("flat_bf16_mirror") == 1
    assert ix.get_stat("flat_half_valid") == ix.get_stat("flat_i8_valid") == (1 if kind == "f32" else 0)
    dst, src = ix.remove_rows(rows)
    for i in sorted(rows.tolist(), reverse=True):
        twin.swap_remove(i)
    assert len(ix) == len(twin) == n1
    assert len(dst) == int((rows < n1).sum()) and (src >= n1).all() and (dst < n1).all()
    got, want = _rows_of(ix, kind == "u8"), _rows_of(twin, kind == "u8")
    assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert np.array_equal(want, base[_replay(n, rows)])  # (and the twin is what the definition says)
    # every kept mirror answers like the twin, whose mirrors are built from scratch
    # queries at refilled holes, at the new end of the table and at removed rows (which must not come back)
    holes = dst[:: max(1, len(dst) // 16)][:16]
    qs = np.concatenate([want[holes.astype(np.int64)], want[n1 - 3:], base[rows[:4]]]).astype(np.float32) + np.float32(0.01)
    twin.set_flat_mode(2)
    for i8, half in tiers:
        for x in (ix, twin):
            x.set_param("flat_i8", i8)
            x.set_param("flat_half", half)
        a, b = ix.flat_knn(qs, 5), twin.flat_knn(qs, 5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (i8, half)
        assert a[0][: len(holes), 0].tolist() == holes.tolist() and a[0][len(holes): len(holes) + 3, 0].tolist() == [n1 - 3, n1 - 2, n1 - 1]
    ix.close()
    twin.close()


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_remove_everything_then_add(mods, kind):
    vdb, O = mods
    rng = np.random.default_rng(12)
    n = 20011
    base, ix, twin = _table(vdb, kind, n, rng)
    twin.close()
    ix.set_flat_mode(2)
    qs = rng.standard_normal((5, ix.dim)).astype(np.float32) * (64 if kind == "u8" else 1)
    ix.flat_knn(qs, 3)  # (mirrors live)
    dst, src = ix.remove_rows(np.arange(n))
    assert len(ix) == 0 and len(dst) == 0 and len(src) == 0
    idx, d, cnt = ix.flat_knn(qs, 3)
    assert cnt.tolist() == [0] * 5
    again = base[100:n - 57]
    if kind == "u8":
        ix.batch_add_u8(again)
    else:
        ix.batch_add(again)
    assert len(ix) == len(again)
    assert np.array_equal(_rows_of(ix, kind == "u8")[:: 997], again[:: 997])
    idx, d, cnt = ix.flat_knn(qs, 3)
    oi, od, oc = O.flat_knn_batch(again.astype(np.float32), qs, 3, 0, nthreads=8)
    assert cnt.tolist() == oc.tolist() and np.array_equal(idx, oi) and np.array_equal(d, od)
    ix.close()


# ---- searches right after the call -------------------------------------------------------------------------------------------------
def _case(O, n, m_random, seed, kinds=(0, 1)):
    """base rows, R (random rows + a block across n' + the first tile's rows), the replayed table, 64 queries that look at the rewritten
    slots (32 moved tail rows, 32 removed rows, + 1e-3 noise), and per metric the oracle's top 12 on the replayed table"""
    rng = np.random.default_rng(seed)
    base = (rng.standard_normal((n, DIM)) + rng.standard_normal(DIM) * 0.5).astype(np.float32)
    rows = set(rng.permutation(n)[:m_random].tolist()) | set(range(2, 9))
    n1_guess = n - len(rows) - 40
    rows |= set(range(n1_guess - 20, n1_guess + 20))
    rows = np.array(sorted(rows))
    keep = _replay(n, rows)
    n1 = len(keep)
    assert n1 % 16 and n1 % 192 and n % 16 and n % 192, (n, n1)
    moved = keep[:n1][keep[:n1] != np.arange(n1)]  # original ids of the rows that now sit in a removed slot
    assert len(moved) >= 32 and (moved >= n1).all()
    qrows = np.concatenate([moved[np.linspace(0, len(moved) - 1, 32).astype(int)], rows[np.linspace(0, len(rows) - 1, 32).astype(int)]])
    qs = (base[qrows] + 1e-3 * rng.standard_normal((64, DIM))).astype(np.float32)
    after = np.ascontiguousarray(base[keep])
    top = {kind: O.flat_knn_batch(after, qs, 12, kind, nthreads=8) for kind in kinds}
    # the moved rows' queries find their row in its NEW slot
    for kind in kinds:
        slot = {int(o): i for i, o in enumerate(keep)}
        assert [int(top[kind][0][q, 0]) for q in range(32)] == [slot[int(o)] for o in qrows[:32]]
    return dict(base=base, rows=rows, after=after, qs=qs, top=top, n1=n1)


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


def _check_searches(ix, case, kind):
    oi, od, oc = case["top"][kind]
    idx, d, cnt = ix.flat_knn(case["qs"], 7)
    assert cnt.tolist() == [7] * 64
    assert np.array_equal(idx, oi[:, :7].astype(np.uint64)), np.nonzero((idx != oi[:, :7]).any(1))
    assert np.array_equal(d.view(np.uint32), od[:, :7].view(np.uint32))
    radius, el, ei, ed = _expect_range(case["top"][kind])
    gl, gi, gd = ix.range_search(case["qs"], radius)
    assert np.array_equal(gl, el) and np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32))


@pytest.fixture(scope="module")
def big_case(mods):
    return _case(mods[1], 22037, 1900, 21)


@pytest.mark.parametrize("dist,kind", [("l2sqr", 0), ("cosine", 1)])
@pytest.mark.parametrize("tier", ["i8", "fp16", "bf16"])
def test_search_after_removal_per_tier(mods, big_case, tier, dist, kind):
    vdb, _ = mods
    c = big_case
    ix = vdb.GpuIndex(DIM, dist)
    ix.batch_add(c["base"])
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", TIERS[tier][0])
    ix.set_param("flat_half", TIERS[tier][1])
    ix.flat_knn(c["qs"], 7)  # the tier's mirror is built and in step with the table
    before = {s: ix.get_stat(s) for s in ("flat_i8_queries", "flat_half_queries")}
    ix.remove_rows(c["rows"])
    assert len(ix) == c["n1"]
    if tier == "i8":
        assert ix.get_stat("flat_i8_valid") == 1  # kept, not dropped for a rebuild
    _check_searches(ix, c, kind)
    if tier == "i8":
        assert ix.get_stat("flat_i8_valid") == 1 and ix.get_stat("flat_i8_queries") >= before["flat_i8_queries"] + 64
    if tier == "fp16":
        assert ix.get_stat("flat_half_queries") >= before["flat_half_queries"] + 64
    ix.close()


@pytest.mark.parametrize("dist,kind", [("l2sqr", 0), ("cosine", 1)])
def test_search_after_removal_small_table(mods, dist, kind):
    """1000 rows, nothing forced: the one-launch kernel / the scan read the rows and the norms themselves"""
    vdb, O = mods
    c = _case(O, 1003, 150, 22, kinds=(kind,))
    ix = vdb.GpuIndex(DIM, dist)
    ix.batch_add(c["base"])
    ix.flat_knn(c["qs"][:4], 7)
    ix.remove_rows(c["rows"])
    _check_searches(ix, c, kind)
    oi, od, _ = c["top"][kind]
    idx, d, cnt = ix.flat_knn(c["qs"][:8], 7)  # (fewer than 32 queries: k_flat_small)
    assert np.array_equal(idx, oi[:8, :7].astype(np.uint64)) and np.array_equal(d, od[:8, :7])
    ix.close()


def test_mirror_keys_equal_the_twins(mods, big_case):
    """fp16 (tier 0) and split-bf16 (tier 1) keys of every remaining row: bulk removal == the swap_remove loop, bit for bit"""
    vdb, _ = mods
    c = big_case
    rows = np.concatenate([c["rows"][::8], c["rows"][-60:]])
    rows = np.unique(rows)
    pair = []
    for _ in range(2):
        ix = vdb.GpuIndex(DIM, "l2sqr")
        ix.batch_add(c["base"])
        ix.set_param("flat_i8", 1)
        ix.prepare(all_tiers=True)
        assert ix.get_stat("flat_half_valid") == 1 and ix.get_stat("flat_bf16_mirror") == 1
        pair.append(ix)
    ix, twin = pair
    ix.remove_rows(rows)
    for i in sorted(rows.tolist(), reverse=True):
        twin.swap_remove(i)
    assert len(ix) == len(twin)
    for tier in (0, 1):
        a = ix.flat_shortlist_keys(c["qs"][28:36], tier)
        b = twin.flat_shortlist_keys(c["qs"][28:36], tier)
        assert a[0].shape == (8, len(ix)) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), tier
        assert a[3] == b[3]  # same scale, same measured error
    ix.close()
    twin.close()


def test_mirror_behind_the_table(mods):
    """batch_add, then remove_rows before any search: the 8-bit mirror is behind, dropped, and rebuilt by the next search"""
    vdb, O = mods
    rng = np.random.default_rng(23)
    n = 20005
    base = rng.standard_normal((n + 33, DIM)).astype(np.float32)
    qs = (base[[3, 77, n + 1, n + 30, 19000]] + 1e-3 * rng.standard_normal((5, DIM))).astype(np.float32)
    ix = vdb.GpuIndex(DIM, "l2sqr")
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.batch_add(base[:n])
    ix.flat_knn(qs, 7)
    assert ix.get_stat("flat_i8_valid") == 1
    ix.batch_add(base[n:])
    rows = np.array([3, 500, 501, n - 1, n + 5])
    ix.remove_rows(rows)
    assert ix.get_stat("flat_i8_valid") == 0
    after = np.ascontiguousarray(base[_replay(n + 33, rows)])
    idx, d, cnt = ix.flat_knn(qs, 7)
    oi, od, oc = O.flat_knn_batch(after, qs, 7, 0, nthreads=8)
    assert cnt.tolist() == oc.tolist() and np.array_equal(idx, oi.astype(np.uint64)) and np.array_equal(d, od)
    assert ix.get_stat("flat_i8_valid") == 1
    ix.close()


def test_masks_go_stale_except_after_an_empty_call(mods):
    vdb, _ = mods
    rng = np.random.default_rng(24)
    base = rng.standard_normal((700, 32)).astype(np.float32)
    ix = vdb.GpuIndex(32, "l2sqr")
    ix.batch_add(base)
    mk = ix.make_mask(np.arange(700) % 2 == 0)
    dst, src = ix.remove_rows([])
    assert len(dst) == 0 and len(ix) == 700
    idx, d, cnt = ix.flat_knn_filtered(base[[0, 2, 4]], 2, mk)  # m == 0: nothing changed, the mask still works
    assert idx[:, 0].tolist() == [0, 2, 4]
    ix.remove_rows([5])
    with pytest.raises(vdb.VdbError, match="error 3"):  # VDB_ERR_STATE
        ix.flat_knn_filtered(base[:3], 2, mk)
    mk.close()
    ix.close()


def test_refusals_leave_the_index_unchanged(mods):
    vdb, _ = mods
    rng = np.random.default_rng(25)
    base = rng.standard_normal((600, 32)).astype(np.float32)
    ix = vdb.GpuIndex(32, "l2sqr")
    ix.batch_add(base)

    def unchanged():
        return len(ix) == 600 and np.array_equal(ix[0], base[0]) and np.array_equal(ix[599], base[599])

    ix.pq_build(n_bits=4, m=8, train_n=200, max_iter=2)
    with pytest.raises(vdb.VdbError, match="swap_remove invalidates the PQ table: clear it first"):
        ix.remove_rows([0, 7])
    ix.pq_clear()
    assert unchanged()
    ix.hnsw_build(M=8, ef_construction=20)
    with pytest.raises(vdb.VdbError, match="swap_remove needs a Flat index"):
        ix.remove_rows([0, 7])
    ix.hnsw_clear()
    assert unchanged()
    ix.ivf_build(8, max_iter=2)
    with pytest.raises(vdb.VdbError, match="swap_remove invalidates the IVF clusters: clear them first"):
        ix.remove_rows([0, 7])
    ix.ivf_clear()
    assert unchanged()
    # invalid lists: out of range, duplicates (caught in Python), and an unsorted list handed to the ABI itself
    with pytest.raises(vdb.VdbError, match="error 1"):
        ix.remove_rows([0, 600])
    for bad_rows in ([4, 4], [-1, 3], [1.5, 2.0], [True, False]):
        with pytest.raises(ValueError):
            ix.remove_rows(bad_rows)
    from lab_1806_vec_db_amd import _lib as L
    bad = np.array([9, 3], dtype=np.uint64)
    moves = C.c_uint64(77)
    assert ix._lib.vdb_index_remove_rows(ix._h, bad.ctypes.data_as(L.u64p), 2, None, None, C.byref(moves)) == 1 and moves.value == 77
    assert unchanged()
    dst, src = ix.remove_rows([0, 7])  # and the index still works
    assert len(ix) == 598 and dst.tolist() == [7, 0] and src.tolist() == [599, 598] and np.array_equal(ix[0], base[598])
    ix.close()
