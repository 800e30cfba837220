"""GPU: scattered label writes (vdb_index_labels_scatter / _device / _set_mask; GpuIndex.set_labels_rows / _device / set_labels_mask;
csrc/k_labels.hip k_labels_scatter / k_labels_set_mask, labels_scatter_plan.hpp).

The model is a numpy (16, n) uint32 array that the test keeps and writes itself.  After every call EVERY column, touched or not, is read
back with get_labels and compared for equality, and label_columns / labels_scatter_calls / labels_scatter_rows are compared with what the
model expects.  Checked: list lengths around the wave and block sizes with row 0 and row n - 1 listed, 1 / 2 / 16 columns in no ascending
order, the codes LABEL_NONE, 0 and 0xFFFFFFFE; lists longer than one launch covers before its grid-stride loop wraps (under a lowered
grid cap at 80 000 rows, and under the default cap on an index that large); columns coming to life; every refusal with state and
counters unchanged; masks built after a write against numpy, masks built before a write still valid and answering as before; writes by
mask from three constructors, empty, all-rows, stale and foreign masks; the device form over torch tensors with ids from flat_knn_device,
a non-zero id_offset and an out-of-range id; a u8 index, remove_rows / batch_add around writes, the 8-bit tier, HNSW and PQ state.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5000
COLS = 16
NONE = 0xFFFFFFFF
SPECIAL = (NONE, 0, 0xFFFFFFFE)
STATS = ("label_columns", "labels_scatter_calls", "labels_scatter_rows")


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    return vdb


def _vecs(n, dim, seed=3):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def _index(vdb, n=N, dim=8):
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(_vecs(n, dim))
    return ix


def _read(ix):
    return np.stack([ix.get_labels(c) for c in range(COLS)])


def _stats(ix):
    return [ix.get_stat(s) for s in STATS]


def _codes(rng, n_cols, m):
    """random codes below 40 with the three special ones among them"""
    c = rng.integers(0, 40, size=(n_cols, m)).astype(np.uint32)
    if c.size:
        flat = c.reshape(-1)
        at = rng.integers(0, flat.size, size=min(flat.size, 3 + flat.size // 7))
        flat[at] = np.array(SPECIAL, dtype=np.uint32)[np.arange(at.size) % 3]
    return c


def _rows(rng, n, m):
    """m distinct rows, shuffled, row 0 and row n - 1 among them when there is room"""
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    if m == 1:
        return np.array([n - 1])
    inner = rng.permutation(np.arange(1, n - 1))[:m - 2]
    return rng.permutation(np.concatenate([[0, n - 1], inner]))


def _check(ix, model, live, calls, rows_written):
    got = _read(ix)
    assert got.dtype == np.uint32 and np.array_equal(got, model)
    assert _stats(ix) == [len(live), calls, rows_written]


# ---- the list form ----------------------------------------------------------------------------------------------------------------------
def test_list_lengths_column_counts_codes_and_new_columns(vdb):
    rng = np.random.default_rng(1806)
    ix = _index(vdb)
    model = np.full((COLS, N), NONE, dtype=np.uint32)
    live, calls, written = set(), 0, 0
    _check(ix, model, live, calls, written)
    column_sets = {1: [[9], [0], [15]], 2: [[7, 2], [15, 0]], 16: [list(rng.permutation(COLS))]}
    for m in (1, 0, 63, 64, 65, 255, 256, 257, 1000, N):
        for n_cols in (1, 2, 16):
            cols = column_sets[n_cols][m % len(column_sets[n_cols])]
            assert n_cols == 1 or cols != sorted(cols)
            rows, codes = _rows(rng, N, m), _codes(rng, n_cols, m)
            if m >= 2:
                assert 0 in rows and N - 1 in rows
            ix.set_labels_rows(rows, cols, codes[0] if n_cols == 1 and m % 2 else codes)  # (1-D codes for one column)
            if m:
                for c, col in enumerate(cols):
                    model[col, rows] = codes[c]
                live |= set(int(c) for c in cols)  # a column never written comes to life, LABEL_NONE on every row not listed
                calls += 1
                written += m
            _check(ix, model, live, calls, written)
    assert len(live) == COLS and all((model == s).any() for s in SPECIAL)
    ix.close()


def test_lists_longer_than_one_launch_covers(vdb):
    rng = np.random.default_rng(7)
    n = 80_000
    ix = _index(vdb, n, 4)
    ix.set_param("labels_scatter_max_blocks", 64)
    span = ix.get_stat("labels_scatter_span")  # from the launcher's own grid computation
    assert span == 64 * 256 and n > 4 * span
    model = np.full((COLS, n), NONE, dtype=np.uint32)
    rows, codes = rng.permutation(n), _codes(rng, 3, n)
    ix.set_labels_rows(rows, [11, 3, 5], codes)
    for c, col in enumerate((11, 3, 5)):
        model[col, rows] = codes[c]
    assert np.array_equal(_read(ix), model)
    mk = ix.make_mask(rng.random(n) < 0.9)  # the write by mask wraps as well
    assert len(mk) > 4 * span
    ix.set_labels_mask(mk, [3, 0], [77, NONE - 1])
    ids = mk.rows()[1]
    model[3, ids], model[0, ids] = 77, NONE - 1
    assert np.array_equal(_read(ix), model)
    mk.close()
    ix.close()
    # the default cap: an index with more rows than one launch covers
    ix = vdb.GpuIndex(4, "l2sqr")
    span = ix.get_stat("labels_scatter_span")
    assert span % 256 == 0 and span >= 256
    n = span + 4097
    ix.batch_add(np.zeros((n, 4), dtype=np.float32))
    rows, codes = rng.permutation(n), rng.integers(0, 2 ** 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
    ix.set_labels_rows(rows, [14, 1], codes)
    for c, col in enumerate((14, 1)):
        want = np.empty(n, dtype=np.uint32)
        want[rows] = codes[c]
        assert np.array_equal(ix.get_labels(col), want)
    assert _stats(ix) == [2, 1, n]
    ix.close()


def test_refusals_leave_columns_and_counters_alone(vdb):
    from lab_1806_vec_db_amd import _lib as L

    rng = np.random.default_rng(11)
    ix = _index(vdb)
    model = np.full((COLS, N), NONE, dtype=np.uint32)
    rows, codes = _rows(rng, N, 700), _codes(rng, 2, 700)
    ix.set_labels_rows(rows, [4, 1], codes)
    model[4, rows], model[1, rows] = codes[0], codes[1]
    live = {1, 4}
    _check(ix, model, live, 1, 700)

    def raw(r, m, cols, n_cols, cd):
        """the C call itself; None: a NULL pointer"""
        r = None if r is None else np.ascontiguousarray(r, dtype=np.uint64)
        cols = None if cols is None else np.ascontiguousarray(cols, dtype=np.uint32)
        cd = None if cd is None else np.ascontiguousarray(cd, dtype=np.uint32)
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return ix._lib.vdb_index_labels_scatter(ix._h, p(r, L.u64p), m, p(cols, L.u32p), n_cols, p(cd, L.u32p))

    two = np.array([5, 9])
    c2 = np.array([[1, 2], [3, 4]], dtype=np.uint32)
    refused = {
        "row_at_n": ([5, N], 2, [4, 7], 2, c2),
        "duplicate_row": ([5, 9, 5], 3, [7], 1, [1, 2, 3]),
        "column_16": (two, 2, [7, 16], 2, c2),
        "column_twice": (two, 2, [7, 7], 2, c2),
        "no_column": (two, 2, [], 0, []),
        "17_columns": (two, 2, np.arange(17) % 16, 17, np.zeros((17, 2))),
        "null_rows": (None, 2, [7], 1, [1, 2]),
        "null_columns": (two, 2, None, 1, [1, 2]),
        "null_codes": (two, 2, [7], 1, None),
    }
    for name, args in refused.items():
        assert raw(*args) == 1, name  # VDB_ERR_INVALID
        assert ix._lib.vdb_last_error(), name
        _check(ix, model, live, 1, 700)  # no column changed, none came to life (7 stays unallocated), no counter moved
    # the same through the Python method: library refusals are VdbError, id validation is update_rows' ValueError
    for r, cols, cd in (([5, N], [4, 7], c2), (two, [7, 16], c2), (two, [7, 7], c2), (two, [], []), (two, np.arange(17) % 16, np.zeros((17, 2)))):
        with pytest.raises(vdb.VdbError, match="error 1"):
            ix.set_labels_rows(r, cols, cd)
    for r in ([5, 9, 5], [True, False, True], [1.0, 2.0, 3.0], [-1, 2, 3]):
        with pytest.raises(ValueError):
            ix.set_labels_rows(r, [7], [1, 2, 3])
    _check(ix, model, live, 1, 700)
    # m == 0 is fine whatever else is given: nothing written, allocated or counted
    assert raw(None, 0, [7], 1, None) == 0 and raw(None, 0, None, 0, None) == 0
    ix.set_labels_rows([], [7, 8], np.zeros((2, 0)))
    _check(ix, model, live, 1, 700)
    ix.close()


# ---- masks and writes -------------------------------------------------------------------------------------------------------------------
def _mask_bits(sel):
    return np.packbits(np.concatenate([sel, np.zeros(-len(sel) % 64, dtype=np.bool_)]), bitorder="little").view(np.uint64)


def test_masks_built_after_a_write_equal_numpy(vdb):
    rng = np.random.default_rng(21)
    ix = _index(vdb)
    model = np.full((COLS, N), NONE, dtype=np.uint32)
    ix.set_labels(2, rng.integers(0, 6, size=N).astype(np.uint32))  # a column written the contiguous way first
    model[2] = ix.get_labels(2)
    for m in (1500, 300):
        rows, codes = _rows(rng, N, m), rng.integers(0, 6, size=(2, m)).astype(np.uint32)
        codes[1, ::5] = NONE
        ix.set_labels_rows(rows, [8, 2], codes)
        model[8, rows], model[2, rows] = codes[0], codes[1]
    assert np.array_equal(_read(ix), model)
    for terms in ([(2, 3)], [(8, 1), (2, 4)], [(8, NONE)], [(2, NONE), (8, 5)]):
        sel = np.ones(N, dtype=np.bool_)
        for col, code in terms:
            sel &= model[col] == code
        mk = ix.make_mask_where(terms)
        words, ids = mk.rows()
        assert np.array_equal(words, _mask_bits(sel)) and np.array_equal(ids, np.flatnonzero(sel)), terms
        mk.close()
    part_codes = [4, NONE, 0, 2]
    parts = ix.make_masks_partition(2, part_codes)
    for code, mk in zip(part_codes, parts):
        words, ids = mk.rows()
        assert np.array_equal(words, _mask_bits(model[2] == code)) and np.array_equal(ids, np.flatnonzero(model[2] == code)), code
    host = ix.make_mask(rng.random(N) < 0.4)
    sel = np.zeros(N, dtype=np.bool_)
    sel[host.rows()[1]] = True
    for col in (2, 8, 5):
        want = [int((model[col] == c).sum()) for c in part_codes]
        assert ix.label_counts(col, part_codes).tolist() == want, col
        assert ix.label_counts(col, part_codes, host).tolist() == [int(((model[col] == c) & sel).sum()) for c in part_codes], col
    for mk in parts + [host]:
        mk.close()
    ix.close()


def test_masks_built_before_a_write_stay_valid(vdb):
    rng = np.random.default_rng(22)
    ix = _index(vdb)
    base = _vecs(N, 8)
    tenant = rng.integers(0, 10, size=N).astype(np.uint32)
    ix.set_labels(0, tenant)
    mk = ix.make_mask_where([(0, 3)])
    words, ids = mk.rows()
    qs = base[:6] + np.float32(0.01)
    before = ix.flat_knn_filtered(qs, 5, mk)
    rows = _rows(rng, N, 2000)
    ix.set_labels_rows(rows, [0, 6], rng.integers(0, 10, size=(2, 2000)).astype(np.uint32))  # moves rows between tenants
    words2, ids2 = mk.rows()  # a mask is a set of rows: not stale, the same set
    assert np.array_equal(words, words2) and np.array_equal(ids, ids2) and np.array_equal(ids, np.flatnonzero(tenant == 3))
    after = ix.flat_knn_filtered(qs, 5, mk)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    ix.set_labels_mask(mk, [0], [9])  # ... and is a valid write list afterwards
    tenant_now = ix.get_labels(0)
    assert (tenant_now[ids] == 9).all()
    mk.close()
    ix.close()


def test_set_labels_mask(vdb):
    rng = np.random.default_rng(23)
    ix = _index(vdb)
    model = np.full((COLS, N), NONE, dtype=np.uint32)
    ix.set_labels(1, rng.integers(0, 4, size=N).astype(np.uint32))
    model[1] = ix.get_labels(1)
    live, calls, written = {1}, 0, 0
    allow = rng.random(N) < 0.3
    allow[[0, N - 1]] = True
    a, b = ix.make_mask(allow), ix.make_mask_where([(1, 2)])
    # (the empty mask first: column 13 must not come to life under it)
    masks = {"empty": ix.make_mask(np.zeros(N, dtype=np.bool_)), "make_mask": a, "where": b, "combine": ix.combine_masks("or", [a, b], [True, False]),
             "all": ix.make_mask(np.ones(N, dtype=np.bool_))}
    writes = {"make_mask": ([12], [5]), "where": ([3, 1], [NONE - 1, 0]), "combine": ([1, 12, 0], [NONE, 7, 8]), "all": (list(range(15, -1, -1)), list(range(100, 116))),
              "empty": ([13], [1])}
    for name, mk in masks.items():
        ids = mk.rows()[1]  # (read before the write: "where" selects by the column it rewrites, and stays the set it was)
        cols, codes = writes[name]
        ix.set_labels_mask(mk, cols, codes)
        if len(ids):
            for col, code in zip(cols, codes):
                model[col, ids] = code
            live |= set(cols)
            calls += 1
            written += len(ids)
        _check(ix, model, live, calls, written)
        assert np.array_equal(mk.rows()[1], ids), name
    assert len(live) == COLS  # ("all" wrote every column)
    # refused: no column over a mask with rows, a column out of range / named twice, a foreign mask, a stale mask
    for cols, codes in (([], []), ([16], [1]), ([2, 2], [1, 1])):
        with pytest.raises(vdb.VdbError, match="error 1"):
            ix.set_labels_mask(a, cols, codes)
    ix.set_labels_mask(masks["empty"], [], [])  # (nothing to write: fine)
    other = _index(vdb)
    foreign = other.make_mask(allow)
    with pytest.raises(vdb.VdbError, match="error 1.*another index"):
        ix.set_labels_mask(foreign, [2], [1])
    _check(ix, model, live, calls, written)
    ix.batch_add(_vecs(3, 8))
    with pytest.raises(vdb.VdbError, match="error 3.*stale"):
        ix.set_labels_mask(a, [2], [1])
    model = np.concatenate([model, np.full((COLS, 3), NONE, dtype=np.uint32)], axis=1)  # the new rows read LABEL_NONE
    _check(ix, model, live, calls, written)
    for mk in list(masks.values()) + [foreign]:
        mk.close()
    other.close()
    ix.close()


# ---- the device form --------------------------------------------------------------------------------------------------------------------
def test_device_form_ids_from_a_search_id_offset_and_bad_ids(vdb):
    import torch

    rng = np.random.default_rng(31)
    dim, off, nq, k = 16, 1000, 16, 10
    base = _vecs(N, dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_id_offset(off)
    model = np.full((COLS, N), NONE, dtype=np.uint32)
    rows, codes = _rows(rng, N, 1000), _codes(rng, 3, 1000)
    d_ids = torch.from_numpy((rows + off).astype(np.int64)).cuda()
    d_codes = torch.from_numpy(codes.view(np.int32)).cuda()
    torch.cuda.synchronize()  # (both arrays complete before the call: it runs on a stream of the library's)
    ix.set_labels_rows_device(d_ids.data_ptr(), 1000, [6, 0, 3], d_codes.data_ptr())
    for c, col in enumerate((6, 0, 3)):
        model[col, rows] = codes[c]
    _check(ix, model, {0, 3, 6}, 1, 1000)
    # ids exactly as flat_knn_device writes them: the k nearest rows of query q get code q in column 9 (rows two queries share get one of
    # the two codes, whole)
    q = torch.from_numpy(base[:nq] + np.float32(1e-3)).cuda()
    idx = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(nq, dtype=torch.int64, device="cuda")
    ix.flat_knn_device(q.data_ptr(), nq, k, idx.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    assert (cnt.cpu().numpy() == k).all()
    hit_codes = torch.arange(nq, dtype=torch.int32, device="cuda").repeat_interleave(k).contiguous()
    torch.cuda.synchronize()
    ix.set_labels_rows_device(idx.data_ptr(), nq * k, [9], hit_codes.data_ptr())
    h_idx = idx.cpu().numpy().astype(np.int64) - off
    got = _read(ix)
    touched = np.zeros(N, dtype=np.bool_)
    touched[h_idx.reshape(-1)] = True
    for r in np.flatnonzero(touched):
        assert got[9, r] in set(np.nonzero((h_idx == r).any(axis=1))[0].tolist()), r
    assert (got[9, ~touched] == NONE).all()
    model[9] = got[9]
    _check(ix, model, {0, 3, 6, 9}, 2, 1000 + nq * k)
    # an id that is no row of the index: refused, nothing written, no column made
    for bad in ([off - 1, off + 5], [off + 5, off + N], [0, off], [off, 2 ** 63]):
        ids = torch.tensor(bad, dtype=torch.int64, device="cuda") if bad[1] < 2 ** 63 else torch.from_numpy(np.array(bad, dtype=np.uint64).view(np.int64)).cuda()
        cd = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
        with pytest.raises(vdb.VdbError, match="error 1.*no row of this index"):
            ix.set_labels_rows_device(ids.data_ptr(), 2, [12], cd.data_ptr())
        _check(ix, model, {0, 3, 6, 9}, 2, 1000 + nq * k)
    with pytest.raises(vdb.VdbError, match="error 1"):
        ix.set_labels_rows_device(d_ids.data_ptr(), 1000, [12, 12], d_codes.data_ptr())
    with pytest.raises(vdb.VdbError, match="error 1"):
        ix.set_labels_rows_device(d_ids.data_ptr(), 1000, [], d_codes.data_ptr())
    ix.set_labels_rows_device(0, 0, [12], 0)  # m == 0
    _check(ix, model, {0, 3, 6, 9}, 2, 1000 + nq * k)
    ix.close()


# ---- other state ------------------------------------------------------------------------------------------------------------------------
def test_u8_index_and_writes_around_remove_rows_and_batch_add(vdb):
    rng = np.random.default_rng(41)
    n = 3000
    ix = vdb.GpuIndex(8, "l2sqr", scalar="u8")
    ix.batch_add_u8(rng.integers(0, 256, size=(n, 8), dtype=np.uint8))
    model = np.full((COLS, n), NONE, dtype=np.uint32)
    rows, codes = _rows(rng, n, 900), _codes(rng, 2, 900)
    ix.set_labels_rows(rows, [5, 2], codes)
    model[5, rows], model[2, rows] = codes[0], codes[1]
    assert np.array_equal(_read(ix), model)
    dst, src = ix.remove_rows(rng.permutation(n)[:400])  # the labels move with the rows
    model[:, dst.astype(np.int64)] = model[:, src.astype(np.int64)]
    model = model[:, :n - 400]
    assert np.array_equal(_read(ix), model)
    ix.batch_add_u8(rng.integers(0, 256, size=(150, 8), dtype=np.uint8))  # the new rows read LABEL_NONE
    model = np.concatenate([model, np.full((COLS, 150), NONE, dtype=np.uint32)], axis=1)
    assert np.array_equal(_read(ix), model)
    n = model.shape[1]
    rows, codes = _rows(rng, n, 1200), _codes(rng, 3, 1200)  # old and new rows, a live and two new columns
    ix.set_labels_rows(rows, [10, 5, 0], codes)
    for c, col in enumerate((10, 5, 0)):
        model[col, rows] = codes[c]
    mk = ix.make_mask(np.arange(n - 150, n))
    ix.set_labels_mask(mk, [2], [3])
    model[2, n - 150:] = 3
    assert np.array_equal(_read(ix), model) and ix.get_stat("label_columns") == 4
    mk.close()
    ix.close()


def test_eight_bit_tier_answers_identically_around_a_write(vdb):
    rng = np.random.default_rng(42)
    n, dim = 20_000, 128
    base = _vecs(n, dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.set_param("flat_half", 0)
    qs = base[:64] + np.float32(0.01)
    before = ix.flat_knn(qs, 7)
    assert ix.get_stat("flat_i8_valid") == 1
    served = ix.get_stat("flat_i8_queries")
    ix.set_labels_rows(rng.permutation(n)[:5000], [1, 0], rng.integers(0, 9, size=(2, 5000)).astype(np.uint32))
    assert ix.get_stat("flat_i8_valid") == 1  # vectors and mirrors are untouched
    after = ix.flat_knn(qs, 7)
    assert ix.get_stat("flat_i8_queries") >= served + 64
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    ix.close()


def test_hnsw_and_pq_state_survive_a_write(vdb):
    rng = np.random.default_rng(43)
    n, dim = 600, 16
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(_vecs(n, dim))
    ix.pq_build(n_bits=4, m=8, train_n=200, seed=7)
    ix.hnsw_build(M=8, ef_construction=40, seed=5)
    assert ix.has_hnsw() and ix.has_pq()
    q = _vecs(4, dim, seed=9)
    before = ix.knn_with_ef(q, 5, 32)
    ix.set_labels_rows(rng.permutation(n)[:200], [0], rng.integers(0, 3, size=200).astype(np.uint32))
    mk = ix.make_mask_where([(0, 1)])
    ix.set_labels_mask(mk, [0, 4], [2, 2])
    mk.close()
    assert ix.has_hnsw() and ix.has_pq()
    after = ix.knn_with_ef(q, 5, 32)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    ix.close()
