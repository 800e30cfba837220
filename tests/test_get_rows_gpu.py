"""GPU: bulk row fetch (vdb_index_get_rows / _u8 / _mask / _device; GpuIndex.get_rows*; csrc/k_fetch.hip, fetch_plan.hpp).

Every vector is compared BIT FOR BIT (uint32 / uint8 views) with the numpy table the test itself keeps; the table holds NaNs with
payloads, +-inf, -0.0 and denormals, so a conversion or a dropped byte shows.  n = 1003 rows.  Checked: every copy width (f32 rows of 4,
12, 400, 512 and 3840 bytes; u8 rows of 3, 100 and 128 bytes, as stored and widened); every list shape with the counters against a
restatement of the plan; chunked calls against the one-chunk call; sentinels around `out` and `d_out`, also for a d_out that is only
4-byte aligned; the table after swap_remove / remove_rows / update_rows / batch_add; id_offset (local rows on the host, global ids on
the device, ids straight from flat_knn_device); masks from three constructors, empty, stale and foreign ones; every refusal with the
output and all four counters untouched; three threads; __getitem__ with a slice and an array.

Not covered: an index past 2^32 elements needs gigabytes and many seconds.  That the row offsets are computed in 64 bits
(`id * row_bytes` in k_rows_gather / k_rows_gather_widen, `rows[0] * out_row` on the direct route) is a code-review item.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1003
STATS = ("fetch_calls", "fetch_rows", "fetch_chunks", "fetch_direct")
SPECIAL = np.array([0x7FC12345, 0xFFC00001, 0x7FA00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], dtype=np.uint32)
SENT = np.float32(-12345.5)
DEFAULT_CHUNK = 128 << 20


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    return vdb


def _base_f32(dim, seed=5):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((N, dim)).astype(np.float32)
    flat = b.reshape(-1).view(np.uint32)
    flat[: len(SPECIAL)] = SPECIAL                     # the first rows
    flat[flat.size - len(SPECIAL):] = SPECIAL[::-1]    # ... and the last
    flat[(N // 2) * dim] = SPECIAL[0]
    return b


def _base_u8(dim, seed=6):
    b = np.random.default_rng(seed).integers(0, 256, size=(N, dim), dtype=np.uint8)
    b[0, :] = 255
    b[N - 1, :] = 0
    return b


def _clean(dim, seed=7, n=N):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def _lists(rng, n=N):
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "one": np.array([n // 3]),
        "last": np.array([n - 1]),
        "all": np.arange(n),
        "subrun": np.arange(17, 400),
        "shuffled": rng.permutation(n),
        "reversed": np.arange(n)[::-1],
        "repeats": rng.integers(0, n, size=2500),
        "same64": np.full(64, n // 2),
    }


def _plan(rows, row_bytes, chunk_bytes):
    """(direct, chunks): the restatement of fetch_plan.hpp"""
    rows = np.asarray(rows, dtype=np.int64)
    m = len(rows)
    run = m >= 1 and bool((rows == rows[0] + np.arange(m)).all())
    cr = max(1, chunk_bytes // row_bytes)
    return run, -(-m // cr)


def _stats(ix):
    return [ix.get_stat(s) for s in STATS]


def _expect(before, rows, row_bytes, chunk_bytes, direct_allowed=True):
    """the counters after one host call over `rows`"""
    m = len(rows)
    if m == 0:
        return before
    run, chunks = _plan(rows, row_bytes, chunk_bytes)
    direct = run and direct_allowed
    return [before[0] + 1, before[1] + m, before[2] + (0 if direct else chunks), before[3] + (1 if direct else 0)]


def _same(a, b):
    va = a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)
    vb = b.view(np.uint8 if b.dtype == np.uint8 else np.uint32)
    return a.shape == b.shape and np.array_equal(va, vb)


# ---- widths x lists -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 100, 128, 960])
def test_f32_widths_and_lists(vdb, dim):
    base = _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    for name, rows in _lists(np.random.default_rng(dim)).items():
        before = _stats(ix)
        got = ix.get_rows(rows)
        assert got.dtype == np.float32 and _same(got, base[rows]), name
        assert _stats(ix) == _expect(before, rows, dim * 4, DEFAULT_CHUNK), name
        if name in ("all", "subrun", "one", "last"):
            assert ix.get_stat("fetch_direct") == before[3] + 1, name
    with pytest.raises(vdb.VdbError):
        ix.get_rows_u8([0])  # as vdb_index_row_u8: a VecSet<u8> index only
    ix.close()


@pytest.mark.parametrize("dim", [3, 100, 128])
def test_u8_widths_and_lists_as_stored_and_widened(vdb, dim):
    base = _base_u8(dim)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar="u8")
    ix.batch_add_u8(base)
    for name, rows in _lists(np.random.default_rng(dim)).items():
        before = _stats(ix)
        got = ix.get_rows_u8(rows)
        assert got.dtype == np.uint8 and _same(got, base[rows]), name
        assert _stats(ix) == _expect(before, rows, dim, DEFAULT_CHUNK), name
        before = _stats(ix)
        wide = ix.get_rows(rows)  # (float)byte, exact; a run is gathered as well: the copy cannot convert
        assert wide.dtype == np.float32 and _same(wide, base[rows].astype(np.float32)), name
        assert _stats(ix) == _expect(before, rows, dim * 4, DEFAULT_CHUNK, direct_allowed=False), name
    ix.close()


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,scalar", [(128, "f32"), (3, "f32"), (100, "u8")])
def test_chunked_calls_equal_the_one_chunk_call(vdb, dim, scalar):
    u8 = scalar == "u8"
    base = _base_u8(dim) if u8 else _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar=scalar)
    (ix.batch_add_u8 if u8 else ix.batch_add)(base)
    rows = np.random.default_rng(3).permutation(N)[:50]
    want = base[rows].astype(np.float32)
    one = ix.get_rows(rows)
    assert _same(one, want)
    for chunk_bytes, chunks in ((1, 50), (7 * dim * 4, 8)):
        ix.set_param("fetch_chunk_bytes", chunk_bytes)
        before = _stats(ix)
        assert _same(ix.get_rows(rows), one)
        assert ix.get_stat("fetch_chunks") - before[2] == chunks and _plan(rows, dim * 4, chunk_bytes) == (False, chunks)
        assert ix.get_stat("fetch_calls") == before[0] + 1 and ix.get_stat("fetch_rows") == before[1] + 50
    ix.set_param("fetch_chunk_bytes", 3 * dim * 4)  # a long list through three rows per chunk: buffers reused many times over
    rows = np.random.default_rng(4).integers(0, N, size=2500)
    before = _stats(ix)
    assert _same(ix.get_rows(rows), base[rows].astype(np.float32))
    assert ix.get_stat("fetch_chunks") - before[2] == 834
    if u8:
        ix.set_param("fetch_chunk_bytes", 7 * dim)
        before = _stats(ix)
        assert _same(ix.get_rows_u8(rows[:50]), base[rows[:50]]) and ix.get_stat("fetch_chunks") - before[2] == 8
    with pytest.raises(vdb.VdbError):
        ix.set_param("fetch_chunk_bytes", 0)
    ix.close()


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shuffled", "subrun", "repeats", "one"])
def test_host_output_inside_sentinels(vdb, name):
    dim = 100
    base = _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    rows = _lists(np.random.default_rng(1))[name]
    big = np.full((len(rows) + 6, dim), SENT, dtype=np.float32)
    out = ix.get_rows(rows, out=big[3:3 + len(rows)])
    assert _same(out, base[rows]) and _same(big[3:3 + len(rows)], base[rows])
    assert (big[:3] == SENT).all() and (big[3 + len(rows):] == SENT).all()
    ix.close()


@pytest.mark.parametrize("dim,scalar,shift", [(128, "f32", 0), (128, "f32", 4), (100, "f32", 0), (3, "f32", 4), (128, "u8", 0), (128, "u8", 4), (3, "u8", 0)])
def test_device_form_inside_sentinels(vdb, dim, scalar, shift):
    """shift = 4: d_out is only 4-byte aligned -- the narrower kernel"""
    import torch

    u8 = scalar == "u8"
    base = _base_u8(dim) if u8 else _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr", scalar=scalar)
    (ix.batch_add_u8 if u8 else ix.batch_add)(base)
    rows = np.random.default_rng(9).integers(0, N, size=1500)
    ids = torch.from_numpy(rows.astype(np.int64)).cuda()
    m = len(rows)
    buf = torch.full(((m + 4) * dim + 1,), float(SENT), dtype=torch.float32, device="cuda")
    first = 2 * dim + shift // 4
    before = _stats(ix)
    ix.get_rows_device(ids.data_ptr(), m, buf.data_ptr() + first * 4)
    assert buf.data_ptr() % 16 == 0 and (dim % 4 or (first * 4) % 16 == shift)  # (the alignment this case is about)
    got = buf.cpu().numpy()
    assert _same(got[first:first + m * dim].reshape(m, dim), base[rows].astype(np.float32))
    assert (got[:first] == SENT).all() and (got[first + m * dim:] == SENT).all()
    assert _stats(ix) == [before[0] + 1, before[1] + m, before[2] + 1, before[3]]
    ix.get_rows_device(0, 0, 0)  # m == 0: nothing is touched, nothing counted
    assert _stats(ix) == [before[0] + 1, before[1] + m, before[2] + 1, before[3]]
    ix.close()


# ---- after writes ---------------------------------------------------------------------------------------------------------------------
def test_fetch_follows_every_write(vdb):
    dim = 100
    rng = np.random.default_rng(11)
    model = _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(model)

    def check():
        rows = rng.permutation(len(model))
        assert len(ix) == len(model) and _same(ix.get_rows(rows), model[rows])

    check()
    ix.swap_remove(5)
    model[5] = model[-1]
    model = model[:-1].copy()
    check()
    dst, src = ix.remove_rows(rng.permutation(len(model))[:120])
    model[dst.astype(np.int64)] = model[src.astype(np.int64)]
    model = model[:len(model) - 120].copy()
    check()
    upd = rng.permutation(len(model))[:77]
    new = rng.standard_normal((77, dim)).astype(np.float32)
    ix.update_rows(upd, new)
    model[upd] = new
    check()
    add = _base_f32(dim, seed=12)[:211]
    ix.batch_add(add)
    model = np.concatenate([model, add])
    check()
    ix.close()


# ---- id_offset ------------------------------------------------------------------------------------------------------------------------
def test_id_offset_local_rows_on_the_host_global_ids_on_the_device(vdb):
    import torch

    dim, off, nq, k = 128, 1000, 16, 10
    base = _clean(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_id_offset(off)
    rows = np.random.default_rng(2).permutation(N)[:300]
    assert _same(ix.get_rows(rows), base[rows])  # local rows, whatever the offset
    ids = torch.from_numpy((rows + off).astype(np.int64)).cuda()
    out = torch.zeros((300, dim), dtype=torch.float32, device="cuda")
    ix.get_rows_device(ids.data_ptr(), 300, out.data_ptr())
    assert _same(out.cpu().numpy(), base[rows])
    # ids straight from a device search
    q = torch.from_numpy(base[:nq] + np.float32(1e-3)).cuda()
    idx = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    dist = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(nq, dtype=torch.int64, device="cuda")
    ix.flat_knn_device(q.data_ptr(), nq, k, idx.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    assert (cnt.cpu().numpy() == k).all()
    hits = torch.zeros((nq * k, dim), dtype=torch.float32, device="cuda")
    ix.get_rows_device(idx.data_ptr(), nq * k, hits.data_ptr())
    h_idx = idx.cpu().numpy().reshape(-1)
    assert h_idx.min() >= off and (h_idx.reshape(nq, k)[:, 0] == np.arange(nq) + off).all()
    assert _same(hits.cpu().numpy(), base[h_idx - off])
    ix.close()


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def test_masks_from_three_constructors_empty_stale_and_foreign(vdb):
    dim = 100
    base = _base_f32(dim)
    rng = np.random.default_rng(13)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    codes = rng.integers(0, 5, size=N).astype(np.uint32)
    ix.set_labels(0, codes)
    allow = rng.random(N) < 0.3
    masks = {"make_mask": ix.make_mask(allow), "where": ix.make_mask_where([(0, 3)]), "all": ix.make_mask(np.ones(N, dtype=np.bool_)),
             "empty": ix.make_mask(np.zeros(N, dtype=np.bool_))}
    parts = ix.make_masks_partition(0, [4, 1, 2])  # views into a slab shared by the three
    masks["partition"] = parts[1]
    want = {"make_mask": np.flatnonzero(allow), "where": np.flatnonzero(codes == 3), "all": np.arange(N), "empty": np.zeros(0, dtype=np.int64),
            "partition": np.flatnonzero(codes == 1)}
    for name, mk in masks.items():
        ids = mk.rows()[1].astype(np.int64)
        assert np.array_equal(ids, want[name]), name
        before = _stats(ix)
        got = ix.get_rows_mask(mk)
        assert got.shape == (len(ids), dim) and _same(got, base[ids]), name
        m = len(ids)
        assert _stats(ix) == ([before[0] + 1, before[1] + m, before[2] + 1, before[3]] if m else before), name
    ix.set_param("fetch_chunk_bytes", 7 * dim * 4)  # the mask's list in chunks
    before = _stats(ix)
    ids = want["make_mask"]
    assert _same(ix.get_rows_mask(masks["make_mask"]), base[ids]) and ix.get_stat("fetch_chunks") - before[2] == -(-len(ids) // 7)
    # a sentinel-framed output
    big = np.full((len(ids) + 4, dim), SENT, dtype=np.float32)
    ix.get_rows_mask(masks["make_mask"], out=big[2:2 + len(ids)])
    assert _same(big[2:2 + len(ids)], base[ids]) and (big[:2] == SENT).all() and (big[2 + len(ids):] == SENT).all()
    # a mask of another index; a mask made stale by batch_add: refused as the filtered searches refuse them, nothing written or counted
    other = vdb.GpuIndex(dim, "l2sqr")
    other.batch_add(base)
    foreign = other.make_mask(allow)
    out = np.full((len(ids), dim), SENT, dtype=np.float32)
    before = _stats(ix)
    with pytest.raises(vdb.VdbError, match="another index"):
        ix.get_rows_mask(foreign, out=out)
    ix.batch_add(base[:3])
    with pytest.raises(vdb.VdbError, match="stale"):
        ix.get_rows_mask(masks["make_mask"], out=out)
    with pytest.raises(vdb.VdbError, match="stale"):
        ix.flat_knn_filtered(_clean(dim)[0], 3, masks["make_mask"])
    assert (out == SENT).all() and _stats(ix) == before
    for mk in list(masks.values()) + parts + [foreign]:
        mk.close()
    other.close()
    ix.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_output_and_counters_alone(vdb):
    import torch
    from lab_1806_vec_db_amd import _lib as L

    dim, off = 128, 1000
    base = _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.get_rows([1, 2, 5])
    before = _stats(ix)
    out = np.full((3, dim), SENT, dtype=np.float32)
    with pytest.raises(vdb.VdbError, match="out of bounds"):
        ix.get_rows([0, N, 1], out=out)  # id == n
    assert (out == SENT).all()
    with pytest.raises(ValueError):
        ix.get_rows([0, -1])
    with pytest.raises(ValueError):
        ix.get_rows([0.5])
    with pytest.raises(ValueError):
        ix.get_rows([True, False])
    with pytest.raises(vdb.VdbError, match="u8"):
        ix.get_rows_u8([0, 1])
    r = np.array([0, 1], dtype=np.uint64)
    assert ix._lib.vdb_index_get_rows(ix._h, r.ctypes.data_as(L.u64p), 2, None) == 1  # null out with m > 0
    assert ix._lib.vdb_index_get_rows(ix._h, None, 2, out.ctypes.data_as(L.f32p)) == 1  # null list with m > 0
    assert ix._lib.vdb_index_get_rows(ix._h, None, 0, None) == 0  # m == 0 touches nothing
    assert (out == SENT).all() and _stats(ix) == before
    # the device form: id == n + offset, id < offset
    ix.set_id_offset(off)
    buf = torch.full((4, dim), float(SENT), dtype=torch.float32, device="cuda")
    for bad in ([off, off + N, off + 1, off + 2], [off + 3, off + 2, off - 1, off], [0, off, off, off]):
        ids = torch.tensor(bad, dtype=torch.int64, device="cuda")
        with pytest.raises(vdb.VdbError, match="no row of this index"):
            ix.get_rows_device(ids.data_ptr(), 4, buf.data_ptr())
        assert (buf.cpu().numpy() == SENT).all()
    ids = torch.tensor([off, off + 1], dtype=torch.int64, device="cuda")
    assert ix._lib.vdb_index_get_rows_device(ix._h, ids.data_ptr(), 2, None, None) == 1  # null d_out
    assert ix._lib.vdb_index_get_rows_device(ix._h, None, 2, buf.data_ptr(), None) == 1  # null d_ids
    assert _stats(ix) == before
    ok = torch.tensor([off + N - 1, off], dtype=torch.int64, device="cuda")  # the same index still answers
    ix.get_rows_device(ok.data_ptr(), 2, buf.data_ptr())
    assert _same(buf.cpu().numpy()[:2], base[[N - 1, 0]]) and (buf.cpu().numpy()[2:] == SENT).all()
    ix.close()


# ---- threads --------------------------------------------------------------------------------------------------------------------------
def test_two_fetching_threads_and_a_searching_one(vdb):
    dim = 128
    base = _clean(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_param("fetch_chunk_bytes", 100 * dim * 4)  # several chunks per call: both staging buffers and the copy stream in use
    q = base[:8] + np.float32(1e-3)
    want_idx, want_dist, _ = ix.flat_knn(q, 5)
    errors = []

    def fetch(seed):
        try:
            rng = np.random.default_rng(seed)
            for _ in range(20):
                rows = rng.permutation(N)
                if not _same(ix.get_rows(rows), base[rows]):
                    errors.append(("fetch", seed))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def search():
        try:
            for _ in range(20):
                idx, dist, _ = ix.flat_knn(q, 5)
                if not (np.array_equal(idx, want_idx) and np.array_equal(dist, want_dist)):
                    errors.append("search")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    before = _stats(ix)
    ts = [threading.Thread(target=fetch, args=(1,)), threading.Thread(target=fetch, args=(2,)), threading.Thread(target=search)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert ix.get_stat("fetch_calls") == before[0] + 40 and ix.get_stat("fetch_rows") == before[1] + 40 * N
    assert ix.get_stat("fetch_chunks") == before[2] + 40 * 11
    ix.close()


# ---- __getitem__ ----------------------------------------------------------------------------------------------------------------------
def test_getitem_int_slice_and_array(vdb):
    dim = 12
    base = _base_f32(dim)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    assert _same(ix[7], base[7]) and ix[7].shape == (dim,)
    for s in (slice(3, 40), slice(None, None, 5), slice(900, None), slice(50, 10, -3), slice(5, 5), slice(-4, None)):
        assert _same(ix[s], base[s]), s
    arr = np.array([5, 5, 1002, 0, 17])
    assert _same(ix[arr], base[arr]) and _same(ix[[3, 1, 2]], base[[3, 1, 2]]) and _same(ix[np.array([-1, 0])], base[[N - 1, 0]])
    with pytest.raises(vdb.VdbError):
        ix[np.array([N])]
    with pytest.raises(IndexError):
        ix[np.array([True, False])]
    ix.close()
