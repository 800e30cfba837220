"""GpuIndex -- host-side mirror of the reference's index traits over the C ABI.

Method names and argument meaning follow src/index_algorithm/mod.rs (IndexIter, IndexKNN, IndexKNNWithEf,
IndexPQ, IndexBuilder) and src/database/dynamic_index.rs:11-94 (DynamicIndex).  All arithmetic runs in
libvdbhip.so on the GPU; this file only marshals numpy arrays.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .labels import LabelTerm

DIST_NAMES = {"l2sqr": L.L2SQR, "cosine": L.COSINE}  # pyo3/mod.rs:15-22


def parse_dist(dist) -> int:
    if isinstance(dist, str):
        try:
            return DIST_NAMES[dist.lower()]
        except KeyError:
            raise ValueError(f"Invalid distance function: {dist}") from None  # PyValueError, pyo3/mod.rs:20
    if dist in (0, 1):
        return int(dist)
    raise ValueError(f"Invalid distance function: {dist}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _nq(queries) -> int:
    """how many queries a host call carries: one when `queries` is a single vector"""
    return 1 if np.ndim(queries) == 1 else len(queries)


def _ptr(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def read_range(lib, h, nq: int):
    """(lims, idx, dist) of a vdb_range result object on the host; releases the object"""
    try:
        lims = np.zeros(nq + 1, dtype=np.uint64)
        L.check(lib.vdb_range_lims(h, _ptr(lims, L.u64p)))
        total = int(lims[nq])
        idx = np.zeros(total, dtype=np.uint64)
        dist = np.zeros(total, dtype=np.float32)
        L.check(lib.vdb_range_copy(h, _ptr(idx, L.u64p), _ptr(dist, L.f32p)))
        return lims, idx, dist
    finally:
        lib.vdb_range_destroy(h)


def pack_mask(allow, n: int) -> np.ndarray:
    """The bit words of a row mask over n rows (vdb_mask_create): row i is allowed iff (words[i >> 6] >> (i & 63)) & 1.
    `allow` is a bool array of length n, or an array of row ids (an id outside [0, n) raises).  Pure host code."""
    n = int(n)
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"mask: a bool array of length {n} is needed, got shape {a.shape}")
        flags = a
    else:
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("mask: a bool array or an array of integer row ids is needed")
        ids = a.reshape(-1).astype(np.int64)
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= n):
            raise ValueError(f"mask: row id out of range for {n} rows")
        flags = np.zeros(n, dtype=np.bool_)
        flags[ids] = True
    nw = (n + 63) // 64
    padded = np.zeros(nw * 64, dtype=np.uint8)
    padded[:n] = flags
    return np.packbits(padded, bitorder="little").view(np.uint64).copy() if nw else np.zeros(0, dtype=np.uint64)


LABEL_COLUMNS = 16         # VDB_LABEL_COLUMNS
LABEL_NONE = 0xFFFFFFFF    # VDB_LABEL_NONE
ROW_NONE = 2 ** 64 - 1     # VDB_ROW_NONE: label_lookup's "no row carries the code"
MASK_MAX_TERMS = 8         # VDB_MASK_MAX_TERMS
MASK_OP_AND, MASK_OP_OR = 0, 1  # VDB_MASK_OP_AND / VDB_MASK_OP_OR
LIKE_MAX_EXAMPLES = 1024   # examples of one query of flat_knn_like, positives plus negatives (LIKE_MAX_EXAMPLES of csrc/like_plan.hpp)
FUSE_MODES = {"rrf": 0, "min": 1}  # VDB_FUSE_RRF / VDB_FUSE_MIN
FUSE_GROUP_MODES = {"rrf": 0, "min": 1, "sum": 2}  # ... and VDB_FUSE_SUM, which only the document-level fusion has
FUSE_MAX_FETCH = 4096      # longest list of flat_knn_fused / fuse_lists_device (FUSE_MAX_FETCH of csrc/fuse_plan.hpp)
MMR_MAX_FETCH = 4096       # longest candidate list of flat_knn_mmr / mmr_select_device (MMR_MAX_FETCH of csrc/mmr_plan.hpp)
FETCH_CHUNK_BYTES_DEFAULT = 128 << 20  # what "fetch_chunk_bytes" is until set_param changes it (Index::FETCH_CHUNK_BYTES_DEFAULT)


def _terms_arrays(terms):
    """(columns, codes) as u32 arrays of a sequence of (column, code) terms"""
    t = [(int(c), int(v)) for c, v in terms]
    for c, v in t:
        if not (0 <= c < 2 ** 32 and 0 <= v < 2 ** 32):
            raise ValueError(f"mask term ({c}, {v}): column and code are u32")
    return (np.array([c for c, _ in t], dtype=np.uint32), np.array([v for _, v in t], dtype=np.uint32))


def _set_terms_arrays(terms):
    """(columns, lo, hi, flags, set_lims, set_words) of a sequence of LabelTerm (an equality term (column, code) stands for its
    LabelTerm equivalent): the arrays of vdb_mask_create_where_sets*, the bitmaps packed back to back"""
    ts = [LabelTerm.of(t) for t in terms]
    maps = [t.bitmap() for t in ts if t.codes is not None]
    lims = [0]
    for t in ts:
        lims.append(lims[-1] + t.set_bits // 64)
    words = maps[0] if len(maps) == 1 else np.concatenate(maps) if maps else np.zeros(0, dtype=np.uint64)
    return (np.array([t.column for t in ts], dtype=np.uint32), np.array([t.lo for t in ts], dtype=np.uint32),
            np.array([t.hi for t in ts], dtype=np.uint32), np.array([t.flags for t in ts], dtype=np.uint32),
            np.array(lims, dtype=np.uint64), words)


def _set_terms_ptrs(arrays):
    """the pointer tail of a set-term call for _set_terms_arrays' tuple (which the caller keeps alive): cols, lo, hi, flags, lims, words"""
    cols, lo, hi, flags, lims, words = arrays
    return (_ptr(cols, L.u32p), _ptr(lo, L.u32p), _ptr(hi, L.u32p), _ptr(flags, L.u32p), _ptr(lims, L.u64p), _ptr(words, L.u64p))


def _lims(lists) -> np.ndarray:
    """the u64 limits of a list of lists: list g is entries [lims[g], lims[g + 1]) of their concatenation"""
    lims = np.zeros(len(lists) + 1, dtype=np.uint64)
    lims[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    return lims


class RowMask:
    """An allow-list over the rows of one GpuIndex (vdb_mask): made by GpuIndex.make_mask, valid until rows are added to or removed
    from the index, closed before the index is."""

    def __init__(self, index: "GpuIndex", words: np.ndarray, n: int):
        self._lib = index._lib
        self._h = L.vp()
        w = np.ascontiguousarray(words, dtype=np.uint64)
        L.check(self._lib.vdb_mask_create(index._h, _ptr(w, L.u64p), int(n), C.byref(self._h)))
        v = C.c_uint64()
        L.check(self._lib.vdb_mask_count(self._h, C.byref(v)))
        self._m = int(v.value)
        self._n = int(n)

    @classmethod
    def from_handle(cls, index: "GpuIndex", handle, n: int | None = None) -> "RowMask":
        """wraps a vdb_mask the library made (vdb_mask_create_where*); the object owns the handle from here on.  `n`: the rows of the
        index, when the caller has them already"""
        self = cls.__new__(cls)
        self._lib = index._lib
        self._h = handle if isinstance(handle, L.vp) else L.vp(handle)
        v = C.c_uint64()
        L.check(self._lib.vdb_mask_count(self._h, C.byref(v)))
        self._m = int(v.value)
        self._n = len(index) if n is None else int(n)
        return self

    def rows(self):
        """(words, ids) of the mask read back from the device (vdb_mask_rows): the u64 bit words over the rows and the u32 ids of the
        allowed rows, ascending"""
        words = np.zeros((self._n + 63) // 64, dtype=np.uint64)
        ids = np.zeros(self._m, dtype=np.uint32)
        L.check(self._lib.vdb_mask_rows(self._h, _ptr(words, L.u64p), _ptr(ids, L.u32p)))
        return words, ids

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.vdb_mask_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return self._m


def calc_dist(a, b, dist="cosine", device: int = 0) -> float:
    """calc_dist (pyo3/mod.rs:43-48), evaluated on the GPU in reference order."""
    kind = parse_dist(dist)
    a, b = _f32(a).ravel(), _f32(b).ravel()
    n = min(a.size, b.size)  # zip truncates (distance/mod.rs:73)
    out = C.c_float(0)
    L.check(L.load().vdb_calc_dist(device, _ptr(a, L.f32p), _ptr(b, L.f32p), n, kind, C.byref(out)))
    return float(out.value)


def calc_dist_u8(a, b, dist="cosine", device: int = 0) -> float:
    """DistanceAdapter<[u8],[u8]> (distance/mod.rs:79-95,106-113): u8 elements widened exactly, f32 folds."""
    kind = parse_dist(dist)
    a = np.ascontiguousarray(a, dtype=np.uint8).ravel()
    b = np.ascontiguousarray(b, dtype=np.uint8).ravel()
    n = min(a.size, b.size)
    out = C.c_float(0)
    L.check(L.load().vdb_calc_dist_u8(device, _ptr(a, L.u8p), _ptr(b, L.u8p), n, kind, C.byref(out)))
    return float(out.value)


class GpuIndex:
    """One HBM-resident VecSet<f32> with optional PQ table and HNSW graph (DynamicIndex + PQTable)."""

    def __init__(self, dim: int, dist="cosine", device: int = 0, scalar: str = "f32"):
        """scalar = "f32" (DynamicIndex) or "u8": a VecSet<u8> held at one byte per element (Flat search only)"""
        self._lib = L.load()
        self._h = L.vp()
        self.device = device
        if scalar not in ("f32", "u8"):
            raise ValueError(f"Invalid scalar type: {scalar}")
        create = self._lib.vdb_index_create_u8 if scalar == "u8" else self._lib.vdb_index_create
        L.check(create(device, int(dim), parse_dist(dist), C.byref(self._h)))

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False):  # (ShardedIndex.local_index: the sharded index owns the handle)
                self._lib.vdb_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- IndexIter ----------------------------------------------------------------------------------
    def __len__(self) -> int:
        v = C.c_uint64()
        L.check(self._lib.vdb_index_len(self._h, C.byref(v)))
        return int(v.value)

    @property
    def dim(self) -> int:
        v = C.c_uint64()
        L.check(self._lib.vdb_index_dim(self._h, C.byref(v)))
        return int(v.value)

    @property
    def dist(self) -> int:
        v = C.c_int()
        L.check(self._lib.vdb_index_dist(self._h, C.byref(v)))
        return int(v.value)

    def __getitem__(self, i) -> np.ndarray:
        """index[i]: one row (vdb_index_row); index[a:b:c] or index[array of row ids]: those rows, (m, dim), through get_rows"""
        if isinstance(i, slice):
            return self.get_rows(np.arange(*i.indices(len(self)), dtype=np.int64))
        if isinstance(i, (np.ndarray, list, tuple)):
            a = np.asarray(i)
            if a.dtype == np.bool_:
                raise IndexError("index[...]: row ids are needed, not a bool mask")
            if a.size and np.issubdtype(a.dtype, np.signedinteger):
                a = np.where(a < 0, a + len(self), a)  # (what is still negative is refused below)
            return self.get_rows(a)
        out = np.empty(self.dim, dtype=np.float32)
        L.check(self._lib.vdb_index_row(self._h, int(i), _ptr(out, L.f32p)))
        return out

    @staticmethod
    def _row_ids(rows, what: str, sort: bool = False, distinct: bool = True) -> np.ndarray:
        """THE check of a host list of local row ids, for the call `what` names in the messages: a flat u64 array of `rows` (ascending
        when `sort`); bool / float / negative ids raise ValueError, and so does a duplicate when `distinct`.  An id at or past len is
        the library's to refuse (VdbError)."""
        a = np.asarray(rows).reshape(-1)
        if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what}: an array of integer row ids is needed")
        if a.size and np.issubdtype(a.dtype, np.signedinteger) and int(a.min()) < 0:
            raise ValueError(f"{what}: negative row id")
        r = np.ascontiguousarray(a.astype(np.uint64))
        if sort or distinct:
            ordered = np.sort(r)
            if distinct and bool((ordered[1:] == ordered[:-1]).any()):
                raise ValueError(f"{what}: duplicate row ids")
            if sort:
                return ordered
        return r

    def get_rows(self, rows, out: np.ndarray | None = None) -> np.ndarray:
        """The vectors of many rows in ONE call (vdb_index_get_rows): (len(rows), dim) f32, row j = local row rows[j]; a u8 index is
        widened.  `rows` in any order, repeats allowed (bool / float / negative ids raise ValueError, an id at or past len VdbError).
        `out`: a C-contiguous float32 array of that shape to fill instead of a new one."""
        r = self._row_ids(rows, "get_rows", distinct=False)
        if out is None:
            out = np.empty((r.size, self.dim), dtype=np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != (r.size, self.dim):
            raise ValueError(f"get_rows: out must be a C-contiguous float32 array of shape {(r.size, self.dim)}")
        L.check(self._lib.vdb_index_get_rows(self._h, _ptr(r, L.u64p), r.size, _ptr(out, L.f32p)))
        return out

    def get_rows_u8(self, rows, out: np.ndarray | None = None) -> np.ndarray:
        """The same for a u8 index, rows as stored: (len(rows), dim) uint8 (vdb_index_get_rows_u8; refused on an f32 index)."""
        r = self._row_ids(rows, "get_rows", distinct=False)
        if out is None:
            out = np.empty((r.size, self.dim), dtype=np.uint8)
        elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.shape != (r.size, self.dim):
            raise ValueError(f"get_rows_u8: out must be a C-contiguous uint8 array of shape {(r.size, self.dim)}")
        L.check(self._lib.vdb_index_get_rows_u8(self._h, _ptr(r, L.u64p), r.size, _ptr(out, L.u8p)))
        return out

    def get_rows_mask(self, mask: "RowMask", out: np.ndarray | None = None) -> np.ndarray:
        """The vectors of the rows a mask allows, ascending by row: (len(mask), dim) f32 (vdb_index_get_rows_mask).  The mask's id list
        on the device is the gather list; a stale mask or one of another index raises VdbError as in the filtered searches."""
        if out is None:
            out = np.empty((len(mask), self.dim), dtype=np.float32)
        elif out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != (len(mask), self.dim):
            raise ValueError(f"get_rows_mask: out must be a C-contiguous float32 array of shape {(len(mask), self.dim)}")
        L.check(self._lib.vdb_index_get_rows_mask(self._h, mask._h, _ptr(out, L.f32p)))
        return out

    def get_rows_device(self, ids_ptr: int, m: int, out_ptr: int, stream: int = 0):
        """Device form (vdb_index_get_rows_device): `ids_ptr` -> m u64 GLOBAL ids on this GPU (row + id_offset, as the *_device searches
        write them), `out_ptr` -> m x dim f32 there (e.g. torch tensor .data_ptr(); any 4-byte alignment).  An id that is no row of the
        index raises VdbError and the output is untouched.  Runs on `stream`, returns synchronised."""
        L.check(self._lib.vdb_index_get_rows_device(self._h, L.vp(ids_ptr), int(m), L.vp(out_ptr), L.vp(stream)))

    # -- IndexBuilder ----------------------------------------------------------------------------------
    def add(self, vec) -> int:
        return self.batch_add(_f32(vec).reshape(1, -1))[0]

    def batch_add(self, rows) -> list[int]:
        rows = _f32(rows)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise L.VdbError(f"dimension mismatch: index dim {self.dim}, got shape {rows.shape}")
        first = C.c_uint64()
        L.check(self._lib.vdb_index_add(self._h, _ptr(rows, L.f32p), rows.shape[0], C.byref(first)))
        return list(range(int(first.value), int(first.value) + rows.shape[0]))

    def add_device(self, data_ptr: int, n: int) -> int:
        """Append n rows already resident on this GPU (e.g. torch tensor .data_ptr())."""
        first = C.c_uint64()
        L.check(self._lib.vdb_index_add_device(self._h, L.vp(data_ptr), int(n), C.byref(first)))
        return int(first.value)

    def swap_remove(self, i: int):
        L.check(self._lib.vdb_index_swap_remove(self._h, int(i)))

    def remove_rows(self, rows):
        """Remove many rows in one call (vdb_index_remove_rows): the state that swap_remove on every row of `rows`, in descending
        order, would leave.  `rows` are local row ids in any order; a duplicate raises ValueError.  Returns (dst, src), u64 arrays: the
        row that was at src[j] is now at dst[j], every other surviving row kept its place -- what a caller needs to permute whatever it
        keeps per row (`meta[dst] = meta[src]`, then truncate)."""
        r = self._row_ids(rows, "remove_rows", sort=True)
        dst = np.zeros(r.size, dtype=np.uint64)
        src = np.zeros(r.size, dtype=np.uint64)
        moves = C.c_uint64()
        L.check(self._lib.vdb_index_remove_rows(self._h, _ptr(r, L.u64p), r.size, _ptr(dst, L.u64p), _ptr(src, L.u64p), C.byref(moves)))
        return dst[:int(moves.value)].copy(), src[:int(moves.value)].copy()

    @classmethod
    def _update_ids(cls, rows) -> np.ndarray:  # (update_rows and the label scatter, whose refusals carry update_rows' name)
        return cls._row_ids(rows, "update_rows")

    def update_rows(self, rows, vecs):
        """New vectors for existing rows, in place (vdb_index_update_rows): row rows[j] gets vecs[j].  `rows` are local row ids in any
        order (bool / float / negative / duplicate ids raise ValueError), `vecs` has shape (len(rows), dim).  Row ids, the row count, the
        label columns and every mask made before the call stay as they are; the mirrors of the Flat tiers are kept in step.  Refused
        (VdbError, index unchanged) under an HNSW graph, a PQ table or IVF clusters, and on a u8 index."""
        r = self._update_ids(rows)
        v = _f32(vecs)
        if r.size == 0 and v.size == 0:
            v = v.reshape(0, self.dim)
        if v.ndim != 2 or v.shape != (r.size, self.dim):
            raise L.VdbError(f"dimension mismatch: index dim {self.dim}, {r.size} rows, got shape {v.shape}")
        L.check(self._lib.vdb_index_update_rows(self._h, _ptr(r, L.u64p), r.size, _ptr(v, L.f32p)))

    def update_rows_device(self, rows, data_ptr: int):
        """The same with the len(rows) x dim f32 vectors already resident on this GPU (e.g. torch tensor .data_ptr(), 16-byte aligned);
        `rows` stays a host array."""
        r = self._update_ids(rows)
        L.check(self._lib.vdb_index_update_rows_device(self._h, _ptr(r, L.u64p), r.size, L.vp(data_ptr)))

    def batch_add_u8(self, rows) -> int:
        """VecSet<u8> rows (widened exactly on the way in, distance/mod.rs:79-95)."""
        r = np.ascontiguousarray(rows, dtype=np.uint8)
        r = r.reshape(1, -1) if r.ndim == 1 else r
        if r.shape[1] != self.dim:
            raise L.VdbError(f"dimension mismatch: index dim {self.dim}, got {r.shape[1]}")
        first = C.c_uint64()
        L.check(self._lib.vdb_index_add_u8(self._h, _ptr(r, L.u8p), r.shape[0], C.byref(first)))
        return int(first.value)

    def row_u8(self, i: int) -> np.ndarray:
        out = np.empty(self.dim, dtype=np.uint8)
        L.check(self._lib.vdb_index_row_u8(self._h, int(i), _ptr(out, L.u8p)))
        return out

    def flat_knn_u8(self, queries, k: int):
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        nq, dim = q.shape
        idx = np.zeros((nq, max(k, 1)), dtype=np.uint64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float32)
        cnt = np.zeros(nq, dtype=np.uint64)
        L.check(self._lib.vdb_flat_knn_u8(self._h, _ptr(q, L.u8p), nq, dim, int(k), _ptr(idx, L.u64p),
                                          _ptr(dist, L.f32p), _ptr(cnt, L.u64p)))
        return idx[:, :k], dist[:, :k], cnt

    def set_id_offset(self, off: int):
        L.check(self._lib.vdb_index_set_id_offset(self._h, int(off)))

    # -- searches ------------------------------------------------------------------------------------------
    @staticmethod
    def _knn_outputs(nq, k):
        """the host outputs of nq queries, zeroed -- (idx, dist) [nq][max(k, 1)] and cnt [nq] -- and the three pointers an entry point takes"""
        kk = max(int(k), 1)
        out = np.zeros((nq, kk), dtype=np.uint64), np.zeros((nq, kk), dtype=np.float32), np.zeros(nq, dtype=np.uint64)
        return out, (_ptr(out[0], L.u64p), _ptr(out[1], L.f32p), _ptr(out[2], L.u64p))

    @staticmethod
    def _knn_cut(out, k):
        """-> (idx [nq][k], dist [nq][k], count [nq]) of _knn_outputs' arrays"""
        return out[0][:, :int(k)], out[1][:, :int(k)], out[2]

    def _knn_call(self, fn, queries, k, *mid):
        """every host k-NN call: fn(handle, queries, nq, dim, k, *mid, idx, dist, cnt) -- `mid`: what the entry point takes between k and the
        outputs (ef; a mask handle; the mask array, its length and mask_of; ...).  One query (1-D): (idx, dist) cut at its count."""
        q = _f32(queries)
        single = q.ndim == 1
        q = q.reshape(1, -1) if single else q
        nq, dim = q.shape
        out, ptrs = self._knn_outputs(nq, k)
        L.check(fn(self._h, _ptr(q, L.f32p), nq, dim, int(k), *mid, *ptrs))
        if single:
            c = int(out[2][0])
            return out[0][0, :c].copy(), out[1][0, :c].copy()
        return self._knn_cut(out, k)

    _search = _knn_call  # (its name before it took more than ef: what the tests of the sharded context compare against)

    def knn(self, queries, k: int):
        """IndexKNN::knn: Flat -> FlatIndex::knn; with an HNSW graph -> HNSWIndex::knn (default ef)
        (dynamic_index.rs:68-73)."""
        if self.has_hnsw():
            return self._knn_call(self._lib.vdb_hnsw_knn, queries, k, 0)
        return self._knn_call(self._lib.vdb_flat_knn, queries, k)

    def flat_knn(self, queries, k: int):
        return self._knn_call(self._lib.vdb_flat_knn, queries, k)

    def make_mask(self, allow) -> RowMask:
        """a row mask for the filtered searches: `allow` is a bool array over the rows or an array of (local) row ids (pack_mask)"""
        n = len(self)
        return RowMask(self, pack_mask(allow, n), n)

    # -- row labels; masks built from them on the device -----------------------------------------------
    def set_labels(self, column: int, codes, first_row: int = 0):
        """rows [first_row, first_row + len(codes)) of label column `column` (vdb_index_labels_set): u32 codes, LABEL_NONE = no value"""
        c = np.ascontiguousarray(np.asarray(codes).reshape(-1), dtype=np.uint32)
        L.check(self._lib.vdb_index_labels_set(self._h, int(column), int(first_row), _ptr(c, L.u32p), c.shape[0]))

    def get_labels(self, column: int, first_row: int = 0, count: int | None = None) -> np.ndarray:
        """the codes of rows [first_row, first_row + count) of one column (to the last row by default); LABEL_NONE where never written"""
        cnt = max(len(self) - int(first_row), 0) if count is None else int(count)
        out = np.zeros(cnt, dtype=np.uint32)
        L.check(self._lib.vdb_index_labels_get(self._h, int(column), int(first_row), cnt, _ptr(out, L.u32p)))
        return out

    @staticmethod
    def _columns_array(columns) -> np.ndarray:
        c = [int(v) for v in np.asarray(columns).reshape(-1).tolist()]
        for v in c:
            if not 0 <= v < 2 ** 32:
                raise ValueError(f"label column {v}: a column is u32")
        return np.array(c, dtype=np.uint32)

    def set_labels_rows(self, rows, columns, codes):
        """Scattered label write (vdb_index_labels_scatter): label column columns[c] of row rows[j] becomes codes[c][j], every column in
        ONE launch.  `rows`: distinct local row ids in any order (bool / float / negative / duplicate ids raise ValueError, as in
        update_rows); `columns`: distinct columns; `codes`: shape (len(columns), len(rows)), or 1-D for one column; LABEL_NONE takes a
        row's value away.  A column never written comes to life first (LABEL_NONE elsewhere).  Masks made before the call stay valid;
        vectors, mirrors, PQ / HNSW / IVF state are untouched.  A refused call (VdbError) changes nothing."""
        r = self._update_ids(rows)
        cols = self._columns_array(columns)
        c = np.ascontiguousarray(codes, dtype=np.uint32)
        if c.ndim == 1 and cols.size == 1:
            c = c.reshape(1, -1)
        elif c.size == 0 and cols.size == 0:  # (no column: the library refuses it when there are rows)
            c = np.zeros((0, r.size), dtype=np.uint32)
        if c.shape != (cols.size, r.size):
            raise ValueError(f"set_labels_rows: codes must have shape {(cols.size, r.size)}, got {c.shape}")
        L.check(self._lib.vdb_index_labels_scatter(self._h, _ptr(r, L.u64p), r.size, _ptr(cols, L.u32p), cols.size, _ptr(c, L.u32p)))

    def set_labels_rows_device(self, ids_ptr: int, m: int, columns, codes_ptr: int):
        """Device form (vdb_index_labels_scatter_device): `ids_ptr` -> m u64 GLOBAL ids on this GPU (row + id_offset, as the *_device
        searches write them; 8-byte aligned), `codes_ptr` -> u32 [len(columns)][m] there; both complete when the call is made.  An id that
        is no row of the index raises VdbError and nothing is written; an id named twice gets one of its codes."""
        cols = self._columns_array(columns)
        L.check(self._lib.vdb_index_labels_scatter_device(self._h, L.vp(ids_ptr), int(m), _ptr(cols, L.u32p), cols.size, L.vp(codes_ptr)))

    def set_labels_mask(self, mask: RowMask, columns, codes):
        """codes[c] into label column columns[c] of EVERY row `mask` allows (vdb_index_labels_set_mask): the mask's id list on the device
        is the write list, nothing is uploaded.  A stale mask or one of another index raises VdbError and nothing changes."""
        cols = self._columns_array(columns)
        c = self._codes_array(np.asarray(codes).reshape(-1).tolist())
        if c.size != cols.size:
            raise ValueError(f"set_labels_mask: one code per column ({cols.size}), got {c.size}")
        L.check(self._lib.vdb_index_labels_set_mask(self._h, mask._h, _ptr(cols, L.u32p), _ptr(c, L.u32p), cols.size))

    def make_mask_where(self, terms) -> RowMask:
        """the mask of the rows whose label in column c equals code for EVERY (c, code) of `terms`, built on the device
        (vdb_mask_create_where); no terms: every row"""
        cols, codes = _terms_arrays(terms)
        h = L.vp()
        L.check(self._lib.vdb_mask_create_where(self._h, _ptr(cols, L.u32p), _ptr(codes, L.u32p), cols.shape[0], C.byref(h)))
        return RowMask.from_handle(self, h)

    def make_masks_where(self, list_of_terms) -> list[RowMask]:
        """one mask per entry of `list_of_terms` (each a sequence of (column, code)) in ONE library call (vdb_mask_create_where_many);
        all-or-nothing: an invalid entry raises and no mask is made"""
        lists = [list(t) for t in list_of_terms]
        lims = _lims(lists)
        cols, codes = _terms_arrays([tm for t in lists for tm in t])
        return self._masks_many(len(lists), lambda arr: self._lib.vdb_mask_create_where_many(
            self._h, _ptr(lims, L.u64p), _ptr(cols, L.u32p), _ptr(codes, L.u32p), len(lists), arr))

    def _masks_many(self, count: int, call, n: int | None = None) -> list[RowMask]:
        """the masks of a library call that fills `count` handles or none: call(handle array) -> status.  `n` as in from_handle"""
        arr = (L.vp * max(count, 1))()
        L.check(call(arr))
        return [RowMask.from_handle(self, arr[g], n) for g in range(count)]

    @staticmethod
    def _codes_array(codes) -> np.ndarray:
        """the u32 array of a sequence of label codes (make_masks_partition, label_counts)"""
        c = [int(v) for v in codes]
        for v in c:
            if not 0 <= v < 2 ** 32:
                raise ValueError(f"label code {v}: a code is u32")
        return np.array(c, dtype=np.uint32)

    def make_masks_partition(self, column: int, codes) -> list[RowMask]:
        """one mask per entry of `codes`: the rows whose label in `column` equals it -- what make_masks_where([[(column, c)] for c in
        codes]) returns, bit for bit, from ONE read of the column per 1024 codes (vdb_mask_create_partition).  The codes are distinct,
        in any order, LABEL_NONE (the unlabelled rows) among them; a duplicate raises and no mask is made.  The masks of a call share
        their device memory by chunks of 1024: it is returned when the last mask of a chunk is closed."""
        c = self._codes_array(codes)
        return self._masks_many(c.shape[0], lambda arr: self._lib.vdb_mask_create_partition(self._h, int(column), _ptr(c, L.u32p), c.shape[0], arr),
                                len(self))

    def label_counts(self, column: int, codes, mask: RowMask | None = None) -> np.ndarray:
        """counts[j] = the number of rows -- of the rows `mask` allows, when one is given -- whose label in `column` equals codes[j], as
        uint64 (vdb_index_label_counts); the same rules for the codes; LABEL_NONE counts the unlabelled rows"""
        c = self._codes_array(codes)
        out = np.zeros(c.shape[0], dtype=np.uint64)
        L.check(self._lib.vdb_index_label_counts(self._h, int(column), None if mask is None else mask._h, _ptr(c, L.u32p), c.shape[0],
                                                 _ptr(out, L.u64p)))
        return out

    @classmethod
    def _lookup_codes(cls, codes) -> np.ndarray:
        """_codes_array, with a vectorised path for an integer array (a lookup may name a million codes)"""
        if isinstance(codes, np.ndarray) and codes.dtype != np.bool_ and np.issubdtype(codes.dtype, np.integer):
            a = codes.reshape(-1)
            if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32):
                raise ValueError("label code out of range: a code is u32")
            return np.ascontiguousarray(a, dtype=np.uint32)
        return cls._codes_array(codes)

    def label_lookup(self, column: int, codes):
        """(first, counts), both uint64 of len(codes): counts[j] = the number of rows whose label in `column` equals codes[j], first[j] =
        the lowest such row, ROW_NONE where there is none (vdb_index_label_lookup) -- from one read of the column when the codes are
        many and dense (the direct route), one per 1024 codes otherwise.  The codes are distinct, in any order, LABEL_NONE (the
        unlabelled rows) among them; a duplicate raises VdbError and nothing is counted."""
        c = self._lookup_codes(codes)
        first = np.full(c.shape[0], ROW_NONE, dtype=np.uint64)
        counts = np.zeros(c.shape[0], dtype=np.uint64)
        L.check(self._lib.vdb_index_label_lookup(self._h, int(column), _ptr(c, L.u32p), c.shape[0], _ptr(first, L.u64p), _ptr(counts, L.u64p)))
        return first, counts

    @classmethod
    def label_lookup_plan(cls, column: int, codes, table_bytes: int = 64 << 20):
        """(route, base, span, chunks) of a label_lookup over `codes` under a scratch cap of table_bytes (vdb_label_lookup_plan; host only,
        no GPU): route 0 = sorted, 1 = direct; base / span over the codes other than LABEL_NONE; chunks = reads of the column.  Raises
        VdbError for what label_lookup refuses."""
        c = cls._lookup_codes(codes)
        route, base, span, chunks = C.c_int(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        L.check(L.load().vdb_label_lookup_plan(int(column), _ptr(c, L.u32p), c.shape[0], int(table_bytes), C.byref(route), C.byref(base),
                                               C.byref(span), C.byref(chunks)))
        return int(route.value), int(base.value), int(span.value), int(chunks.value)

    @staticmethod
    def _dup_limit(limit) -> int:
        if limit is not None and int(limit) <= 0:
            raise ValueError("limit must be positive (None: no limit)")
        return int(limit or 0)

    def dup_groups(self, radius: float, mask: RowMask | None = None, limit: int | None = None):
        """Near-duplicate groups of the index's own rows (vdb_flat_dup_groups): (group, stats).  Row i's neighbours are the rows
        range_search(query = row i, radius, limit, mask) lists; every listed j != i is an undirected edge; the groups are the connected
        components of the allowed rows (all rows, or the mask's) under these edges.  This is SINGLE LINKAGE at the radius: A-B and B-C put
        A and C into one group even when d(A, C) > radius.  group: uint64 [len], the LOWEST row of row i's group + id_offset (its own id
        for a row alone), ROW_NONE for a row outside the mask.  stats: dict with `groups` (of at least 2 rows), `rows` (in them), `pairs`
        (non-self pairs seen) and `truncated` (rows whose list reached `limit`: with a limit a group is a subset of a true component,
        never a union of two).  A NaN radius and a stale or foreign mask raise VdbError."""
        group = np.full(len(self), ROW_NONE, dtype=np.uint64)
        stats = np.zeros(4, dtype=np.uint64)
        L.check(self._lib.vdb_flat_dup_groups(self._h, float(radius), self._dup_limit(limit), None if mask is None else mask._h,
                                              _ptr(group, L.u64p), _ptr(stats, L.u64p)))
        return group, dict(zip(("groups", "rows", "pairs", "truncated"), (int(x) for x in stats)))

    def dup_groups_device(self, radius: float, out_group_ptr: int, mask: RowMask | None = None, limit: int | None = None, stream: int = 0):
        """the same with the group ids written to device memory (u64 [len], 8-byte aligned; vdb_flat_dup_groups_device); returns the
        stats dict, synchronised"""
        stats = np.zeros(4, dtype=np.uint64)
        L.check(self._lib.vdb_flat_dup_groups_device(self._h, float(radius), self._dup_limit(limit), None if mask is None else mask._h,
                                                     L.vp(out_group_ptr), _ptr(stats, L.u64p), L.vp(stream)))
        return dict(zip(("groups", "rows", "pairs", "truncated"), (int(x) for x in stats)))

    def link_pairs_device(self, src_ptr: int, lims_ptr: int, ids_ptr: int, nq: int, out_group_ptr: int, stream: int = 0):
        """the component stage alone over a caller-supplied CSR edge list on the device (vdb_link_pairs_device): src u64 [nq] the ids of
        the lists' source rows, lims u64 [nq + 1] ascending from 0, ids u64 [lims[nq]] (row + id_offset, as the range calls write them),
        out_group u64 [len]: the lowest row of each row's component + id_offset (single linkage over the listed pairs).  Limits that
        descend or an id that is no row of this index raise and leave the output untouched.  Returns the stats dict (truncated = 0)."""
        stats = np.zeros(4, dtype=np.uint64)
        L.check(self._lib.vdb_link_pairs_device(self._h, L.vp(src_ptr), L.vp(lims_ptr), L.vp(ids_ptr), int(nq), L.vp(out_group_ptr),
                                                _ptr(stats, L.u64p), L.vp(stream)))
        return dict(zip(("groups", "rows", "pairs", "truncated"), (int(x) for x in stats)))

    @staticmethod
    def dup_plan(n_rows: int, dim: int, radius: float, m_allowed: int | None = None, chunk: int = 16384, elem_u8: bool = False,
                 limit: int | None = None):
        """(chunks, last, gather, scratch_bytes) of a dup_groups call (vdb_dup_plan; host only, no GPU): the range calls it makes, the
        queries of the last one, whether the queries are gathered (a mask -- m_allowed given -- or u8 rows) and the device bytes held
        besides one chunk's range result.  Raises VdbError for what dup_groups refuses by its arguments (a NaN radius, a bad chunk)."""
        masked = m_allowed is not None
        chunks, last, gather, scratch = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint64()
        L.check(L.load().vdb_dup_plan(int(n_rows), int(dim), int(bool(elem_u8)), int(masked), int(m_allowed if masked else n_rows), float(radius),
                                      int(limit or 0), int(chunk), C.byref(chunks), C.byref(last), C.byref(gather), C.byref(scratch)))
        return int(chunks.value), int(last.value), bool(gather.value), int(scratch.value)

    def make_mask_where_sets(self, terms) -> RowMask:
        """the mask of the rows that match EVERY LabelTerm of `terms` -- set and range predicates over the label columns, built on the
        device (vdb_mask_create_where_sets); no terms: every row"""
        a = _set_terms_arrays(terms)
        h = L.vp()
        L.check(self._lib.vdb_mask_create_where_sets(self._h, *_set_terms_ptrs(a), a[0].shape[0], C.byref(h)))
        return RowMask.from_handle(self, h)

    def make_masks_where_sets(self, list_of_terms) -> list[RowMask]:
        """one mask per entry of `list_of_terms` (each a sequence of LabelTerm) in ONE library call (vdb_mask_create_where_sets_many);
        all-or-nothing: an invalid entry raises and no mask is made"""
        lists = [list(t) for t in list_of_terms]
        tlims = _lims(lists)
        a = _set_terms_arrays([tm for t in lists for tm in t])
        return self._masks_many(len(lists), lambda arr: self._lib.vdb_mask_create_where_sets_many(
            self._h, _ptr(tlims, L.u64p), *_set_terms_ptrs(a), len(lists), arr))

    def make_mask_where_any(self, clauses) -> RowMask:
        """the mask of the rows that match every LabelTerm of SOME clause of `clauses` (a sequence of sequences of LabelTerm) -- an OR of
        conjunctions over the label columns, built on the device in one pass (vdb_mask_create_where_any).  No clauses: the empty mask;
        a clause without terms: every row"""
        cl = [list(c) for c in clauses]
        clims = _lims(cl)
        a = _set_terms_arrays([tm for c in cl for tm in c])
        h = L.vp()
        L.check(self._lib.vdb_mask_create_where_any(self._h, _ptr(clims, L.u64p), len(cl), *_set_terms_ptrs(a), C.byref(h)))
        return RowMask.from_handle(self, h)

    def make_masks_where_any(self, list_of_clause_lists) -> list[RowMask]:
        """one mask per entry of `list_of_clause_lists` (each what make_mask_where_any takes) in ONE library call
        (vdb_mask_create_where_any_many); all-or-nothing: an invalid entry raises and no mask is made"""
        masks = [[list(c) for c in clauses] for clauses in list_of_clause_lists]
        mlims = _lims(masks)
        cl = [c for m in masks for c in m]
        clims = _lims(cl)
        a = _set_terms_arrays([tm for c in cl for tm in c])
        return self._masks_many(len(masks), lambda arr: self._lib.vdb_mask_create_where_any_many(
            self._h, _ptr(mlims, L.u64p), _ptr(clims, L.u64p), *_set_terms_ptrs(a), len(masks), arr))

    def combine_masks(self, op, masks, invert=None) -> RowMask:
        """the AND (op "and" / MASK_OP_AND) or OR ("or" / MASK_OP_OR) of 1 .. 8 masks of this index, mask i complemented within the
        rows first where invert[i] is true, computed on the device (vdb_mask_combine).  One mask with invert=[True] is NOT.  The inputs
        may come from any constructor; a stale mask or one of another index raises"""
        code = {"and": MASK_OP_AND, "or": MASK_OP_OR}.get(op.lower(), -1) if isinstance(op, str) else int(op)
        ms = list(masks)
        arr = (L.vp * max(len(ms), 1))(*[m._h for m in ms])
        inv = None
        if invert is not None:
            inv = np.ascontiguousarray([bool(x) for x in invert], dtype=np.uint8)
            if inv.shape[0] != len(ms):
                raise ValueError(f"combine_masks: {len(ms)} masks, {inv.shape[0]} invert flags")
        h = L.vp()
        L.check(self._lib.vdb_mask_combine(self._h, code, arr, None if inv is None else _ptr(inv, L.u8p), len(ms), C.byref(h)))
        return RowMask.from_handle(self, h)

    def flat_knn_filtered(self, queries, k: int, mask: RowMask):
        """Exact k-NN over the mask's allowed rows alone (vdb_flat_knn_filtered): the first min(k, len(mask)) pairs of flat_knn
        restricted to them, distances bit-exact, ascending by (distance, id); same return shapes as flat_knn."""
        return self._knn_call(self._lib.vdb_flat_knn_filtered, queries, k, mask._h)

    def flat_knn_filtered_device(self, q_ptr: int, nq: int, k: int, mask: RowMask, out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int,
                                 stream: int = 0):
        L.check(self._lib.vdb_flat_knn_filtered_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), mask._h, L.vp(out_idx_ptr),
                                                       L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    @staticmethod
    def _mask_args(masks, mask_of, nq: int):
        """(the vdb_mask* array, its length, mask_of as contiguous u32) of a call with one mask per query"""
        masks = list(masks)
        mo = np.ascontiguousarray(np.asarray(mask_of).reshape(-1), dtype=np.uint32)
        if mo.shape[0] != nq:
            raise ValueError(f"mask_of: one entry per query is needed ({nq}), got {mo.shape[0]}")
        arr = (L.vp * max(len(masks), 1))(*[mk._h for mk in masks])
        return arr, len(masks), mo

    def flat_knn_filtered_multi(self, queries, k: int, masks, mask_of):
        """flat_knn_filtered with ONE MASK PER QUERY (vdb_flat_knn_filtered_multi): query q is answered under masks[mask_of[q]], exactly
        as flat_knn_filtered(queries[q], k, masks[mask_of[q]]) answers it; the buckets of short masks share one scan launch.  `masks`: a
        sequence of RowMask of this index, `mask_of`: nq indexes into it, in any order.  Same return shapes as flat_knn_filtered."""
        arr, n_masks, mo = self._mask_args(masks, mask_of, _nq(queries))
        return self._knn_call(self._lib.vdb_flat_knn_filtered_multi, queries, k, arr, n_masks, _ptr(mo, L.u32p))

    def flat_knn_filtered_multi_device(self, q_ptr: int, nq: int, k: int, masks, mask_of, out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int,
                                       stream: int = 0):
        arr, n_masks, mo = self._mask_args(masks, mask_of, int(nq))
        L.check(self._lib.vdb_flat_knn_filtered_multi_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), arr, n_masks, _ptr(mo, L.u32p),
                                                             L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def _grouped_mask_args(self, masks, mask_of, nq: int):
        """(array, count, mask_of pointer) of a grouped call: no masks = unfiltered; one mask without mask_of = that mask for every query"""
        if masks is None:
            return None, 0, None, None
        if isinstance(masks, RowMask):
            masks = [masks]
        if mask_of is None:
            masks = list(masks)
            if len(masks) != 1:
                raise ValueError("mask_of is needed with more than one mask")
            mask_of = np.zeros(nq, dtype=np.uint32)
        arr, n_masks, mo = self._mask_args(masks, mask_of, nq)
        return arr, n_masks, _ptr(mo, L.u32p), mo

    def flat_knn_grouped(self, queries, k: int, column: int, group_size: int = 1, masks=None, mask_of=None):
        """Exact k-NN with at most `group_size` hits per value of label column `column` (vdb_flat_knn_grouped): per query the first k rows,
        in flat_knn's order, such that fewer than group_size earlier rows of that order carry the same label; rows without a label are
        always kept.  masks=None: over all rows; otherwise query q under masks[mask_of[q]] as in flat_knn_filtered_multi (one RowMask and
        no mask_of: that mask for every query).  Same return shapes as flat_knn_filtered."""
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, _nq(queries))
        return self._knn_call(self._lib.vdb_flat_knn_grouped, queries, k, int(column), int(group_size), arr, n_masks, mo_p)

    def flat_knn_grouped_device(self, q_ptr: int, nq: int, k: int, column: int, group_size: int, out_idx_ptr: int, out_dist_ptr: int,
                                out_cnt_ptr: int, masks=None, mask_of=None, stream: int = 0):
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, int(nq))
        L.check(self._lib.vdb_flat_knn_grouped_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(column), int(group_size), arr, n_masks,
                                                      mo_p, L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def group_cap_device(self, ids_ptr: int, dists_ptr: int, counts_ptr: int, nq: int, ld: int, k: int, column: int, group_size: int,
                         out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int, stream: int = 0):
        """the capped walk alone over caller-supplied device lists [nq][ld] (u64 ids, f32 distances) and u64 counts, walked in the order
        given (vdb_group_cap_device); an id that is no row of this index raises and leaves the outputs untouched"""
        L.check(self._lib.vdb_group_cap_device(self._h, L.vp(ids_ptr), L.vp(dists_ptr), L.vp(counts_ptr), int(nq), int(ld), int(k), int(column),
                                               int(group_size), L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def flat_knn_mmr(self, queries, k: int, fetch_k: int, lambda_mult: float = 0.5, masks=None, mask_of=None):
        """Diversified exact k-NN, maximal marginal relevance (vdb_flat_knn_mmr): per query, from the first min(fetch_k, allowed rows)
        rows of flat_knn's order, the nearest row and then greedily the row with the smallest
        lambda_mult * d(query, row) - (1 - lambda_mult) * min over the selected rows of d(row, selected), ties to the earlier row; the hits
        come IN SELECTION ORDER with the distances of flat_knn.  k <= fetch_k <= 4096, 0 <= lambda_mult <= 1 (1: flat_knn itself, 0:
        farthest-first among the candidates).  masks / mask_of as in flat_knn_grouped.  Same return shapes as flat_knn_filtered."""
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, _nq(queries))
        return self._knn_call(self._lib.vdb_flat_knn_mmr, queries, k, int(fetch_k), float(lambda_mult), arr, n_masks, mo_p)

    def flat_knn_mmr_device(self, q_ptr: int, nq: int, k: int, fetch_k: int, lambda_mult: float, out_idx_ptr: int, out_dist_ptr: int,
                            out_cnt_ptr: int, masks=None, mask_of=None, stream: int = 0):
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, int(nq))
        L.check(self._lib.vdb_flat_knn_mmr_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(fetch_k), float(lambda_mult), arr, n_masks,
                                                  mo_p, L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def mmr_select_device(self, ids_ptr: int, dists_ptr: int, counts_ptr: int, nq: int, ld: int, k: int, lambda_mult: float,
                          out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int, stream: int = 0):
        """the greedy selection alone over caller-supplied device lists [nq][ld] (u64 ids, f32 distances; ld <= 4096, k <= ld) and u64
        counts, walked in the order given: position 0 is selected first and position is the tie order (vdb_mmr_select_device); an id that
        is no row of this index raises and leaves the outputs untouched"""
        L.check(self._lib.vdb_mmr_select_device(self._h, L.vp(ids_ptr), L.vp(dists_ptr), L.vp(counts_ptr), int(nq), int(ld), int(k),
                                                float(lambda_mult), L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    @staticmethod
    def _fuse_args(lims, mode, weights, modes=FUSE_MODES):
        """(lims u64, mode code, weights f32 or None) of a fused call; `mode` is a name of `modes` or the library's code"""
        lm = np.ascontiguousarray(lims, dtype=np.uint64).ravel()
        if lm.size == 0:
            raise ValueError("lims: nq + 1 entries are needed")
        code = modes.get(mode, mode) if isinstance(mode, str) else int(mode)
        if isinstance(code, str):
            raise ValueError(f"fusion mode {mode!r}: " + " or ".join(repr(m) for m in modes))
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
            if w.size != int(lm[-1]):
                raise ValueError(f"{w.size} weights for {int(lm[-1])} sub-queries")
        return lm, code, w

    def flat_knn_fused(self, queries, lims, k: int, fetch_k: int, mode="rrf", weights=None, rrf_c: float = 60.0, masks=None, mask_of=None):
        """Fused multi-query exact search (vdb_flat_knn_fused): fused query q owns the sub-queries lims[q] .. lims[q + 1] - 1 of `queries`
        (1 to 32 each); each sub-query contributes the first min(fetch_k, allowed rows) rows of flat_knn's order and the lists are joined
        on the device.  mode="rrf": score = the f32 left fold over the sub-queries, ascending, of weight / ((rank + 1) + rrf_c), hits by
        score descending (ties: ascending id), `dist` carries the score.  mode="min": the smallest distance over the sub-queries, hits
        ascending -- for fetch_k >= k exactly the k rows nearest to any sub-query; weights must be None.  masks / mask_of as in
        flat_knn_grouped, indexed by SUB-query.  k <= fetch_k <= 4096, sub-queries x fetch_k <= 16384.
        -> (idx [nq][k], dist [nq][k], count [nq]); slots past a count are zero."""
        lm, code, w = self._fuse_args(lims, mode, weights)
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        if q.shape[0] != int(lm[-1]):
            raise ValueError(f"{q.shape[0]} query vectors for {int(lm[-1])} sub-queries")
        nq = lm.size - 1
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, q.shape[0])
        out, ptrs = self._knn_outputs(nq, k)
        L.check(self._lib.vdb_flat_knn_fused(self._h, _ptr(q, L.f32p), _ptr(lm, L.u64p), nq, q.shape[1], int(k), int(fetch_k), code, _ptr(w, L.f32p),
                                             float(rrf_c), arr, n_masks, mo_p, *ptrs))
        return self._knn_cut(out, k)

    def flat_knn_fused_device(self, q_ptr: int, lims, k: int, fetch_k: int, out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int, mode="rrf",
                              weights=None, rrf_c: float = 60.0, masks=None, mask_of=None, stream: int = 0):
        """Device form (vdb_flat_knn_fused_device): lims and weights on the host, the sub-queries' vectors and the outputs on this GPU, at
        most 32768 sub-queries"""
        lm, code, w = self._fuse_args(lims, mode, weights)
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, int(lm[-1]))
        L.check(self._lib.vdb_flat_knn_fused_device(self._h, L.vp(q_ptr), _ptr(lm, L.u64p), lm.size - 1, self.dim, int(k), int(fetch_k), code,
                                                    _ptr(w, L.f32p), float(rrf_c), arr, n_masks, mo_p, L.vp(out_idx_ptr), L.vp(out_dist_ptr),
                                                    L.vp(out_cnt_ptr), L.vp(stream)))

    def fuse_lists_device(self, ids_ptr: int, dists_ptr: int, counts_ptr: int, lims, ld: int, k: int, out_idx_ptr: int, out_dist_ptr: int,
                          out_cnt_ptr: int, mode="rrf", weights=None, rrf_c: float = 60.0, stream: int = 0):
        """the fusion alone over caller-supplied device lists [lims[-1]][ld] (u64 ids, f32 distances; ld <= 4096) and u64 counts, walked in
        the order given: position is the rank, and of an id that occurs twice in one list only the first occurrence counts
        (vdb_fuse_lists_device); an id that is no row of this index raises and leaves the outputs untouched"""
        lm, code, w = self._fuse_args(lims, mode, weights)
        L.check(self._lib.vdb_fuse_lists_device(self._h, L.vp(ids_ptr), L.vp(dists_ptr), L.vp(counts_ptr), _ptr(lm, L.u64p), lm.size - 1, int(ld),
                                                int(k), code, _ptr(w, L.f32p), float(rrf_c), L.vp(out_idx_ptr), L.vp(out_dist_ptr),
                                                L.vp(out_cnt_ptr), L.vp(stream)))

    @staticmethod
    def fuse_groups_plan(lims, k: int, fetch_k: int, mode="rrf", weights=None, rrf_c: float = 60.0, column: int = 0, budget: int = 0):
        """vdb_fuse_groups_plan, no GPU needed -> (code, s_max, table_lg, in_lds, scratch bytes per fused query, sub-chunk); code 0: the
        search forms accept the call, and only then are the others meaningful (they are None otherwise)"""
        lm = np.ascontiguousarray(lims, dtype=np.uint64).ravel()
        code = FUSE_GROUP_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).ravel()
        rc, in_lds, lg = C.c_int(-1), C.c_int(-1), C.c_uint32(0)
        s_max, scratch, sub = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(L.load().vdb_fuse_groups_plan(code, _ptr(lm, L.u64p) if lm.size else None, max(lm.size, 1) - 1, int(k), int(fetch_k), _ptr(w, L.f32p),
                                              float(rrf_c), int(column), int(budget), C.byref(rc), C.byref(s_max), C.byref(lg), C.byref(in_lds),
                                              C.byref(scratch), C.byref(sub)))
        if rc.value:
            return rc.value, None, None, None, None, None
        return 0, s_max.value, lg.value, in_lds.value, scratch.value, sub.value

    def flat_knn_fused_groups(self, queries, lims, k: int, fetch_k: int, column: int, mode="rrf", weights=None, rrf_c: float = 60.0, masks=None,
                              mask_of=None, return_exact: bool = False):
        """Document-level fused exact search (vdb_flat_knn_fused_groups): flat_knn_fused with the lists joined by GROUP -- the rows that
        share a value of label column `column`; a row without one is a group of its own.  Per list a group counts once, at its first
        (nearest) row.  mode="rrf": the f32 left fold of weight / ((rank among the list's groups + 1) + rrf_c), descending; "min": the
        smallest such distance, ascending; "sum": the fold, over every non-empty list, of that distance -- or of the list's last distance
        where the list does not hold the group -- ascending (late interaction; a lower bound of the true sum while a list is cut at
        fetch_k).  `idx` carries each group's representative row (its nearest), `dist` the score.
        -> (idx [nq][k], dist [nq][k], count [nq]), and with return_exact a u8 array [nq]: whether the whole table would give this answer."""
        lm, code, w = self._fuse_args(lims, mode, weights, FUSE_GROUP_MODES)
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        if q.shape[0] != int(lm[-1]):
            raise ValueError(f"{q.shape[0]} query vectors for {int(lm[-1])} sub-queries")
        nq = lm.size - 1
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, q.shape[0])
        out, ptrs = self._knn_outputs(nq, k)
        exact = np.zeros(max(nq, 1), dtype=np.uint8)
        L.check(self._lib.vdb_flat_knn_fused_groups(self._h, _ptr(q, L.f32p), _ptr(lm, L.u64p), nq, q.shape[1], int(k), int(fetch_k), code,
                                                    _ptr(w, L.f32p), float(rrf_c), int(column), arr, n_masks, mo_p, *ptrs,
                                                    _ptr(exact, L.u8p) if return_exact else None))
        res = self._knn_cut(out, k)
        return res + (exact[:nq],) if return_exact else res

    def flat_knn_fused_groups_device(self, q_ptr: int, lims, k: int, fetch_k: int, column: int, out_idx_ptr: int, out_dist_ptr: int,
                                     out_cnt_ptr: int, out_exact_ptr: int = 0, mode="rrf", weights=None, rrf_c: float = 60.0, masks=None,
                                     mask_of=None, stream: int = 0):
        """Device form (vdb_flat_knn_fused_groups_device): lims and weights on the host, the sub-queries' vectors and the outputs (exact: u8,
        0 = not wanted) on this GPU, at most 32768 sub-queries"""
        lm, code, w = self._fuse_args(lims, mode, weights, FUSE_GROUP_MODES)
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, int(lm[-1]))
        L.check(self._lib.vdb_flat_knn_fused_groups_device(self._h, L.vp(q_ptr), _ptr(lm, L.u64p), lm.size - 1, self.dim, int(k), int(fetch_k), code,
                                                           _ptr(w, L.f32p), float(rrf_c), int(column), arr, n_masks, mo_p, L.vp(out_idx_ptr),
                                                           L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(out_exact_ptr), L.vp(stream)))

    def fuse_groups_device(self, ids_ptr: int, dists_ptr: int, counts_ptr: int, lims, ld: int, k: int, column: int, out_idx_ptr: int,
                           out_dist_ptr: int, out_cnt_ptr: int, out_exact_ptr: int = 0, mode="rrf", weights=None, rrf_c: float = 60.0,
                           trunc_len: int | None = None, stream: int = 0):
        """the document-level fusion alone over caller-supplied device lists [lims[-1]][ld] (u64 ids, f32 distances; ld <= 4096) and u64
        counts, walked in the order given; a list that counts `trunc_len` entries (default ld, at least 1) or more is a truncated one
        (vdb_fuse_groups_device); an id that is no row of this index raises and leaves the outputs untouched"""
        lm, code, w = self._fuse_args(lims, mode, weights, FUSE_GROUP_MODES)
        tl = max(int(ld), 1) if trunc_len is None else int(trunc_len)
        L.check(self._lib.vdb_fuse_groups_device(self._h, L.vp(ids_ptr), L.vp(dists_ptr), L.vp(counts_ptr), _ptr(lm, L.u64p), lm.size - 1, int(ld),
                                                 int(k), code, _ptr(w, L.f32p), float(rrf_c), int(column), tl, L.vp(out_idx_ptr), L.vp(out_dist_ptr),
                                                 L.vp(out_cnt_ptr), L.vp(out_exact_ptr), L.vp(stream)))

    @staticmethod
    def _like_lists(lists, nq=None):
        """(lims, ids) of a list of id lists as u64 arrays: query q's ids are ids[lims[q]:lims[q + 1]]; None -> (None, None)"""
        if lists is None:
            return None, None
        lists = [np.asarray(x, dtype=np.uint64).ravel() for x in lists]
        if nq is not None and len(lists) != nq:
            raise ValueError(f"{len(lists)} id lists for {nq} queries")
        lims = _lims(lists)
        ids = np.concatenate(lists).astype(np.uint64) if lists else np.zeros(0, dtype=np.uint64)
        return lims, np.ascontiguousarray(ids)

    def like_queries(self, positives, negatives=None):
        """The query vectors of a search by example rows (vdb_like_queries): `positives` / `negatives` are lists of LOCAL row id lists,
        one per query (negatives=None: none).  Per element, in f32: the strict left fold of a query's positive rows in list order divided
        by their number, ap; with negatives an likewise and (ap + ap) - an.  -> float32 [nq][dim]."""
        pl, pr = self._like_lists(positives)
        nq = len(pl) - 1
        nl, nr = self._like_lists(negatives, nq)
        out = np.zeros((nq, self.dim), dtype=np.float32)
        L.check(self._lib.vdb_like_queries(self._h, _ptr(pl, L.u64p), _ptr(pr, L.u64p), _ptr(nl, L.u64p), _ptr(nr, L.u64p), nq, _ptr(out, L.f32p)))
        return out

    def like_queries_device(self, pos_lims, pos_ids_ptr: int, neg_lims, neg_ids_ptr: int, nq: int, out_ptr: int, stream: int = 0):
        """Device form (vdb_like_queries_device): `pos_lims` / `neg_lims` are HOST u64 arrays of nq + 1 limits (neg_lims None: no
        negatives), the id pointers -> u64 GLOBAL ids (row + id_offset) on this GPU, `out_ptr` -> nq x dim f32 there: a valid query
        pointer for every *_device search.  An id that is no row of the index raises and leaves the output untouched."""
        pl = np.ascontiguousarray(pos_lims, dtype=np.uint64)
        nl = None if neg_lims is None else np.ascontiguousarray(neg_lims, dtype=np.uint64)
        L.check(self._lib.vdb_like_queries_device(self._h, _ptr(pl, L.u64p), L.vp(pos_ids_ptr), _ptr(nl, L.u64p), L.vp(neg_ids_ptr), int(nq),
                                                  L.vp(out_ptr), L.vp(stream)))

    def flat_knn_like(self, positives, k: int, negatives=None, exclude: bool = True, masks=None, mask_of=None):
        """Exact search by example rows (vdb_flat_knn_like): per query the k nearest allowed rows, in flat_knn's order, of the query vector
        like_queries makes from its `positives` / `negatives` (lists of LOCAL row id lists, at least one positive and at most 1024
        examples per query); exclude=True leaves every example out of the answer.  masks / mask_of as in flat_knn_grouped.
        -> (idx [nq][k], dist [nq][k], count [nq]); slots past a count are zero."""
        pl, pr = self._like_lists(positives)
        nq = len(pl) - 1
        nl, nr = self._like_lists(negatives, nq)
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, nq)
        out, ptrs = self._knn_outputs(nq, k)
        L.check(self._lib.vdb_flat_knn_like(self._h, _ptr(pl, L.u64p), _ptr(pr, L.u64p), _ptr(nl, L.u64p), _ptr(nr, L.u64p), nq, int(k),
                                            int(bool(exclude)), arr, n_masks, mo_p, *ptrs))
        return self._knn_cut(out, k)

    def flat_knn_like_device(self, pos_lims, pos_ids_ptr: int, neg_lims, neg_ids_ptr: int, nq: int, k: int, out_idx_ptr: int,
                             out_dist_ptr: int, out_cnt_ptr: int, exclude: bool = True, masks=None, mask_of=None, stream: int = 0):
        """Device form (vdb_flat_knn_like_device): limits on the host, u64 GLOBAL ids and the outputs on this GPU, at most 32768 queries"""
        pl = np.ascontiguousarray(pos_lims, dtype=np.uint64)
        nl = None if neg_lims is None else np.ascontiguousarray(neg_lims, dtype=np.uint64)
        arr, n_masks, mo_p, _keep = self._grouped_mask_args(masks, mask_of, int(nq))
        L.check(self._lib.vdb_flat_knn_like_device(self._h, _ptr(pl, L.u64p), L.vp(pos_ids_ptr), _ptr(nl, L.u64p), L.vp(neg_ids_ptr), int(nq),
                                                   int(k), int(bool(exclude)), arr, n_masks, mo_p, L.vp(out_idx_ptr), L.vp(out_dist_ptr),
                                                   L.vp(out_cnt_ptr), L.vp(stream)))

    def drop_listed_device(self, ids_ptr: int, dists_ptr: int, counts_ptr: int, nq: int, ld: int, k: int, drop_lims, drop_ids_ptr: int,
                           out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int, stream: int = 0):
        """the compaction alone over caller-supplied device lists [nq][ld] (u64 ids, f32 distances) and u64 counts, walked in the order
        given (vdb_drop_listed_device): per query the first k entries whose id is not among drop_ids[drop_lims[q]:drop_lims[q + 1]]
        (HOST limits, u64 global ids on the device, at most 1024 per query); an id that is no row of this index raises and leaves the
        outputs untouched"""
        dl = np.ascontiguousarray(drop_lims, dtype=np.uint64)
        L.check(self._lib.vdb_drop_listed_device(self._h, L.vp(ids_ptr), L.vp(dists_ptr), L.vp(counts_ptr), int(nq), int(ld), int(k),
                                                 _ptr(dl, L.u64p), L.vp(drop_ids_ptr), L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr),
                                                 L.vp(stream)))

    def _range_out(self, h, nq: int):
        return read_range(self._lib, h, nq)

    @staticmethod
    def _range_args(queries, radius, limit):
        """(queries as [nq][dim] f32, nq, dim, one radius per query as f32, limit as the C calls take it: 0 = none) of a host range call"""
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        nq, dim = q.shape
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,)))
        if limit is not None and int(limit) <= 0:
            raise ValueError("limit must be positive (None: no limit)")
        return q, nq, dim, r, int(limit or 0)

    def range_search(self, queries, radius, limit: int | None = None, mask: RowMask | None = None):
        """Exact Flat range search (vdb_flat_range): for every query ALL rows with distance <= its radius -- the distance
        FlatIndex::knn computes, boundary included -- ascending by (distance, index); with `limit` the first `limit` of them,
        i.e. search(k = limit, upper_bound = radius).  `radius`: one value, or one per query.
        Returns (lims, idx, dist): query q owns idx / dist [lims[q], lims[q + 1])."""
        q, nq, dim, r, limit = self._range_args(queries, radius, limit)
        h = L.vp()
        if mask is not None:  # only the mask's allowed rows (vdb_flat_range_filtered)
            L.check(self._lib.vdb_flat_range_filtered(self._h, _ptr(q, L.f32p), nq, dim, _ptr(r, L.f32p), limit, mask._h,
                                                      C.byref(h)))
            return self._range_out(h, nq)
        L.check(self._lib.vdb_flat_range(self._h, _ptr(q, L.f32p), nq, dim, _ptr(r, L.f32p), limit, C.byref(h)))
        return self._range_out(h, nq)

    def range_search_device(self, q_ptr: int, nq: int, radius_ptr: int, limit: int | None = None, stream: int = 0):
        """the same with device-resident queries (f32 [nq][dim]) and radii (f32 [nq]); returns synchronised, results on the host"""
        h = L.vp()
        L.check(self._lib.vdb_flat_range_device(self._h, L.vp(q_ptr), int(nq), self.dim, L.vp(radius_ptr), int(limit or 0),
                                                L.vp(stream), C.byref(h)))
        return self._range_out(h, int(nq))

    def range_search_multi(self, queries, radius, masks, mask_of, limit: int | None = None):
        """range_search with ONE MASK PER QUERY (vdb_flat_range_filtered_multi): query q's slice is what
        range_search(queries[q], radius[q], limit, mask=masks[mask_of[q]]) returns; the buckets of short masks share one scan launch.
        `radius`: one value, or one per query; `masks`: a sequence of RowMask of this index, `mask_of`: nq indexes into it, in any
        order.  Returns (lims, idx, dist) as range_search does."""
        q, nq, dim, r, limit = self._range_args(queries, radius, limit)
        arr, n_masks, mo = self._mask_args(masks, mask_of, nq)
        h = L.vp()
        L.check(self._lib.vdb_flat_range_filtered_multi(self._h, _ptr(q, L.f32p), nq, dim, _ptr(r, L.f32p), limit, arr, n_masks,
                                                        _ptr(mo, L.u32p), C.byref(h)))
        return self._range_out(h, nq)

    def range_search_multi_device(self, q_ptr: int, nq: int, radius_ptr: int, masks, mask_of, limit: int | None = None, stream: int = 0):
        """the same with device-resident queries (f32 [nq][dim]) and radii (f32 [nq]); returns synchronised, results on the host"""
        arr, n_masks, mo = self._mask_args(masks, mask_of, int(nq))
        h = L.vp()
        L.check(self._lib.vdb_flat_range_filtered_multi_device(self._h, L.vp(q_ptr), int(nq), self.dim, L.vp(radius_ptr), int(limit or 0), arr,
                                                               n_masks, _ptr(mo, L.u32p), L.vp(stream), C.byref(h)))
        return self._range_out(h, int(nq))

    def knn_with_ef(self, queries, k: int, ef: int):
        """IndexKNNWithEf::knn_with_ef; Flat ignores ef (dynamic_index.rs:75-80)."""
        if self.has_hnsw():
            return self._knn_call(self._lib.vdb_hnsw_knn, queries, k, int(ef))
        return self._knn_call(self._lib.vdb_flat_knn, queries, k)

    def knn_pq(self, queries, k: int, ef: int):
        """IndexPQ::knn_pq (dynamic_index.rs:82-93)."""
        if self.has_hnsw():
            return self._knn_call(self._lib.vdb_hnsw_knn_pq, queries, k, int(ef))
        return self._knn_call(self._lib.vdb_flat_knn_pq, queries, k, int(ef))

    def flat_knn_device(self, q_ptr: int, nq: int, k: int, out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int,
                        stream: int = 0):
        L.check(self._lib.vdb_flat_knn_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), L.vp(out_idx_ptr),
                                              L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def flat_knn_device_begin(self, q_ptr: int, nq: int, k: int, out_idx_ptr: int, out_dist_ptr: int, out_cnt_ptr: int,
                              stream: int = 0):
        """first half of flat_knn_device (vdb_flat_knn_device_begin): enqueues the search behind `stream` and returns a pending
        handle for flat_knn_device_end; keep two batches in flight to pipeline independent query batches"""
        h = L.vp()
        L.check(self._lib.vdb_flat_knn_device_begin(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), L.vp(out_idx_ptr),
                                                    L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream), C.byref(h)))
        return h

    def flat_knn_device_end(self, pending):
        """second half: waits for the call, redoes uncertified queries, frees the handle; outputs valid on return"""
        L.check(self._lib.vdb_flat_knn_device_end(pending))

    def knn_pq_device(self, q_ptr: int, nq: int, k: int, ef: int, out_idx_ptr: int, out_dist_ptr: int,
                      out_cnt_ptr: int, stream: int = 0):
        L.check(self._lib.vdb_flat_knn_pq_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(ef),
                                                 L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr),
                                                 L.vp(stream)))

    def hnsw_knn_device(self, q_ptr: int, nq: int, k: int, ef: int, out_idx_ptr: int, out_dist_ptr: int,
                        out_cnt_ptr: int, use_pq: bool = False, stream: int = 0):
        L.check(self._lib.vdb_hnsw_knn_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(ef), int(use_pq),
                                              L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    def merge_topk_device(self, d_dists: int, d_ids: int, d_counts: int, n_shards: int, nq: int, k: int,
                          out_idx: int, out_dist: int, out_cnt: int, stream: int = 0):
        L.check(self._lib.vdb_merge_topk_device(self._h, L.vp(d_dists), L.vp(d_ids), L.vp(d_counts), n_shards, nq, k,
                                                L.vp(out_idx), L.vp(out_dist), L.vp(out_cnt), L.vp(stream)))

    def range_merge_device(self, d_lims: int, d_ids: int, d_dists: int, n_shards: int, nq: int, pair_stride: int,
                           limit: int | None = None, stream: int = 0):
        """Merge of S range results on this index's GPU (vdb_range_merge_device): device pointers to lims [S][nq + 1] (u64), ids
        (u64) and distances (f32) with shard s's pairs at element s * pair_stride -- the all-gathered tensors.  Returns the merged
        (lims, idx, dist) on the host like range_search; synchronises `stream` first."""
        if limit is not None and int(limit) <= 0:
            raise ValueError("limit must be positive (None: no limit)")
        h = L.vp()
        L.check(self._lib.vdb_range_merge_device(self._h, L.vp(d_lims), L.vp(d_ids), L.vp(d_dists), int(n_shards), int(nq),
                                                 int(pair_stride), int(limit or 0), L.vp(stream), C.byref(h)))
        return self._range_out(h, int(nq))

    # -- row-sharded knn_pq: local ADC shortlist as pair-key rows, merged after the all-gather ------
    def knn_pq_shard(self, queries, k: int, ef: int):
        """This shard's ADC top-max(ef,k): (adc_keys, exact_keys), each [nq, max(ef,k)] uint64 with GLOBAL ids."""
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        efk = max(int(ef), int(k))
        adc = np.full((q.shape[0], efk), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        ex = np.full((q.shape[0], efk), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        L.check(self._lib.vdb_flat_knn_pq_shard(self._h, _ptr(q, L.f32p), q.shape[0], q.shape[1], int(k), int(ef),
                                                _ptr(adc, L.u64p), _ptr(ex, L.u64p)))
        return adc, ex

    def knn_pq_shard_device(self, q_ptr: int, nq: int, k: int, ef: int, out_adc_ptr: int, out_exact_ptr: int,
                            stream: int = 0):
        L.check(self._lib.vdb_flat_knn_pq_shard_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(ef),
                                                       L.vp(out_adc_ptr), L.vp(out_exact_ptr), L.vp(stream)))

    def pq_merge_resort_device(self, d_adc: int, d_exact: int, n_shards: int, nq: int, efk: int, k: int,
                               out_idx: int, out_dist: int, out_cnt: int, stream: int = 0):
        L.check(self._lib.vdb_pq_merge_resort_device(self._h, L.vp(d_adc), L.vp(d_exact), n_shards, nq, efk, k,
                                                     L.vp(out_idx), L.vp(out_dist), L.vp(out_cnt), L.vp(stream)))

    def merge_topk_gathered(self, d_gathered: int, block_bytes: int, off_ids: int, off_dists: int, off_counts: int,
                            n_shards: int, nq: int, k: int, out_idx: int, out_dist: int, out_cnt: int, stream: int = 0):
        L.check(self._lib.vdb_merge_topk_gathered(self._h, L.vp(d_gathered), block_bytes, off_ids, off_dists, off_counts,
                                                  n_shards, nq, k, L.vp(out_idx), L.vp(out_dist), L.vp(out_cnt),
                                                  L.vp(stream)))

    def merge_topk_gathered_async(self, d_gathered: int, block_bytes: int, off_ids: int, off_dists: int, off_counts: int,
                                  n_shards: int, nq: int, k: int, out_idx: int, out_dist: int, out_cnt: int, stream: int):
        """vdb_merge_topk_gathered_async: the merge enqueued on `stream`, no host synchronisation (k <= 64)"""
        L.check(self._lib.vdb_merge_topk_gathered_async(self._h, L.vp(d_gathered), block_bytes, off_ids, off_dists, off_counts,
                                                        n_shards, nq, k, L.vp(out_idx), L.vp(out_dist), L.vp(out_cnt),
                                                        L.vp(stream)))

    def flat_shortlist_keys(self, queries, tier: int):
        """approximate keys of the Flat shortlist pass for every row (vdb_flat_shortlist_keys): (keys [nq, len], qsq [nq],
        qerr [nq], dict(dx_abs, dx_rel, xsq_max, xsq_min_pos)); tier 0 = fp16 operands, 1 = split-bf16 operands"""
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        keys = np.zeros((q.shape[0], len(self)), dtype=np.float32)
        qsq = np.zeros(q.shape[0], dtype=np.float32)
        qerr = np.zeros(q.shape[0], dtype=np.float32)
        dx = np.zeros(4, dtype=np.float32)
        L.check(self._lib.vdb_flat_shortlist_keys(self._h, _ptr(q, L.f32p), q.shape[0], q.shape[1], int(tier), _ptr(keys, L.f32p),
                                                  _ptr(qsq, L.f32p), _ptr(qerr, L.f32p), _ptr(dx, L.f32p)))
        return keys, qsq, qerr, {"dx_abs": float(dx[0]), "dx_rel": float(dx[1]), "xsq_max": float(dx[2]), "xsq_min_pos": float(dx[3])}

    def prepare(self, all_tiers: bool = False):
        """build now the operand mirrors the first Flat search would build (vdb_index_prepare); all_tiers: those of the redo tiers too"""
        L.check(self._lib.vdb_index_prepare(self._h, 1 if all_tiers else 0))

    def set_flat_mode(self, mode: int):
        L.check(self._lib.vdb_flat_set_mode(self._h, int(mode)))

    def set_param(self, name: str, value: int):
        L.check(self._lib.vdb_set_param(self._h, name.encode(), int(value)))

    def flat_fallback_count(self) -> int:
        v = C.c_uint64()
        L.check(self._lib.vdb_flat_fallback_count(self._h, C.byref(v)))
        return int(v.value)

    def get_stat(self, name: str) -> int:
        v = C.c_uint64()
        L.check(self._lib.vdb_get_stat(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    # -- PQ ------------------------------------------------------------------------------------------------
    def pq_attach(self, n_bits: int, m: int, centroids, codes=None):
        """PQTable fields (pq_table.rs:116-137) as arrays: centroids = (1 << n_bits) * dim floats in group order,
        codes = len x ceil(m * n_bits / 8) bytes or None (encoded on the GPU).  Sizes are checked here: the C side
        copies exactly that many elements."""
        c = _f32(centroids).ravel()
        cd = None if codes is None else np.ascontiguousarray(codes, dtype=np.uint8)
        if n_bits not in (4, 8):
            raise L.VdbError("n_bits must be 4 or 8 in PQTable.")
        if not 0 < int(m) <= self.dim:
            raise L.VdbError("m must be in 1..=dim")
        if c.size != (1 << n_bits) * self.dim:
            raise L.VdbError(f"pq_attach: centroids hold {c.size} floats, expected (1 << n_bits) * dim = {(1 << n_bits) * self.dim}")
        enc = (int(m) + 1) // 2 if n_bits == 4 else int(m)
        if cd is not None and cd.size != len(self) * enc:
            raise L.VdbError(f"pq_attach: codes hold {cd.size} bytes, expected len * encoded_dim = {len(self) * enc}")
        L.check(self._lib.vdb_pq_attach(self._h, n_bits, m, _ptr(c, L.f32p), _ptr(cd, L.u8p)))

    def pq_build(self, n_bits: int = 4, m: int | None = None, train_n: int = 0, max_iter: int = 20,
                 tol: float = 1e-6, seed: int = 42):
        m = -(-self.dim // 3) if m is None else m
        L.check(self._lib.vdb_pq_build(self._h, n_bits, m, train_n, max_iter, tol, seed))

    def pq_clear(self):
        L.check(self._lib.vdb_pq_clear(self._h))

    def has_pq(self) -> bool:
        v = C.c_int()
        L.check(self._lib.vdb_pq_has(self._h, C.byref(v)))
        return bool(v.value)

    def pq_export(self):
        nb, m, ed = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(self._lib.vdb_pq_info(self._h, C.byref(nb), C.byref(m), C.byref(ed)))
        cent = np.zeros((1 << nb.value) * self.dim, dtype=np.float32)
        codes = np.zeros((len(self), ed.value), dtype=np.uint8)
        L.check(self._lib.vdb_pq_export(self._h, _ptr(cent, L.f32p), _ptr(codes, L.u8p)))
        return {"n_bits": int(nb.value), "m": int(m.value), "centroids": cent, "codes": codes}

    def pq_create_lookup(self, queries):
        """PQTable::create_lookup (pq_table.rs:195-224): (lut [nq, m * k_c], dist_cache [nq]) as the search kernels build them."""
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        nb, m, ed = C.c_uint64(), C.c_uint64(), C.c_uint64()
        L.check(self._lib.vdb_pq_info(self._h, C.byref(nb), C.byref(m), C.byref(ed)))
        lut = np.zeros((q.shape[0], m.value << nb.value), dtype=np.float32)
        qc = np.zeros(q.shape[0], dtype=np.float32)
        L.check(self._lib.vdb_pq_create_lookup(self._h, _ptr(q, L.f32p), q.shape[0], q.shape[1], _ptr(lut, L.f32p), _ptr(qc, L.f32p)))
        return lut, qc

    def pq_adc_all(self, queries):
        """ADC distance of every code row to every query (pq_table.rs:239-301): [nq, len] float32."""
        q = _f32(queries)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        out = np.zeros((q.shape[0], len(self)), dtype=np.float32)
        L.check(self._lib.vdb_pq_adc_all(self._h, _ptr(q, L.f32p), q.shape[0], q.shape[1], _ptr(out, L.f32p)))
        return out

    # -- HNSW ------------------------------------------------------------------------------------------------
    def hnsw_build(self, M: int = 16, ef_construction: int = 200, seed: int = 42, batch: int = 1,
                   nthreads: int = 1):
        L.check(self._lib.vdb_hnsw_build(self._h, M, ef_construction, seed, batch, nthreads))

    def hnsw_attach(self, M: int, ef_construction: int, g: dict):
        l0 = np.ascontiguousarray(g["level0"], dtype=np.uint32)
        len0 = np.ascontiguousarray(g["len0"], dtype=np.uint64)
        vl = np.ascontiguousarray(g["vec_level"], dtype=np.uint64)
        up = np.ascontiguousarray(g["upper"], dtype=np.uint32)
        ul = np.ascontiguousarray(g["upper_len"], dtype=np.uint64)
        # the C side reads n * max_m0 / n / n / sum(vec_level) * m / sum(vec_level) elements: check before it does
        n, mm = len(self), min(int(M), 10000)
        tot = int(vl.sum()) if vl.size == n else -1
        if l0.size != n * 2 * mm or len0.size != n or vl.size != n or up.size != tot * mm or ul.size != tot:
            raise L.VdbError(f"hnsw_attach: array sizes do not match len={n}, M={M}: level0 {l0.size}, len0 {len0.size}, "
                             f"vec_level {vl.size}, upper {up.size}, upper_len {ul.size}")
        L.check(self._lib.vdb_hnsw_attach(self._h, M, ef_construction, _ptr(l0, L.u32p), _ptr(len0, L.u64p),
                                          _ptr(vl, L.u64p), _ptr(up, L.u32p), _ptr(ul, L.u64p),
                                          int(g["has_enter"]), int(g["enter_point"]), int(g["enter_level"])))

    def hnsw_clear(self):
        L.check(self._lib.vdb_hnsw_clear(self._h))

    def has_hnsw(self) -> bool:
        v = C.c_int()
        L.check(self._lib.vdb_hnsw_has(self._h, C.byref(v)))
        return bool(v.value)

    def hnsw_export(self) -> dict:
        m, mm0, tot, ep, el, de = (C.c_uint64() for _ in range(6))
        he = C.c_int()
        L.check(self._lib.vdb_hnsw_info(self._h, C.byref(m), C.byref(mm0), C.byref(tot), C.byref(he), C.byref(ep),
                                        C.byref(el), C.byref(de)))
        n = len(self)
        g = {
            "n": n, "m": int(m.value), "max_m0": int(mm0.value),
            "level0": np.zeros(n * mm0.value, dtype=np.uint32), "len0": np.zeros(n, dtype=np.uint64),
            "vec_level": np.zeros(n, dtype=np.uint64), "upper": np.zeros(tot.value * m.value, dtype=np.uint32),
            "upper_len": np.zeros(tot.value, dtype=np.uint64), "has_enter": int(he.value),
            "enter_point": int(ep.value), "enter_level": int(el.value), "default_ef": int(de.value),
        }
        L.check(self._lib.vdb_hnsw_export(self._h, _ptr(g["level0"], L.u32p), _ptr(g["len0"], L.u64p),
                                          _ptr(g["vec_level"], L.u64p), _ptr(g["upper"], L.u32p),
                                          _ptr(g["upper_len"], L.u64p)))
        return g

    def hnsw_last_stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        L.check(self._lib.vdb_hnsw_last_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # -- IVF (index_algorithm/ivf_index.rs) ---------------------------------------------------------------------
    def ivf_build(self, k: int, train_n: int = 0, max_iter: int = 20, tol: float = 1e-6, seed: int = 42):
        """IVFIndex::from_vec_set with IVFConfig{k, k_means_size, k_means_max_iter, k_means_tol} (ivf_index.rs:19-31)."""
        L.check(self._lib.vdb_ivf_build(self._h, int(k), int(train_n), int(max_iter), float(tol), int(seed)))

    def ivf_attach(self, centroids, assign=None):
        c = _f32(centroids)
        a = None if assign is None else np.ascontiguousarray(assign, dtype=np.uint64)
        if c.ndim != 2 or c.shape[1] != self.dim:
            raise L.VdbError(f"ivf_attach: centroids must be k x dim = ? x {self.dim}, got {c.shape}")
        if a is not None and a.size != len(self):
            raise L.VdbError(f"ivf_attach: assign holds {a.size} entries, expected len = {len(self)}")
        L.check(self._lib.vdb_ivf_attach(self._h, c.shape[0], _ptr(c.ravel(), L.f32p), _ptr(a, L.u64p)))

    def ivf_clear(self):
        L.check(self._lib.vdb_ivf_clear(self._h))

    def ivf_info(self):
        p, k, d = C.c_int(), C.c_uint64(), C.c_uint64()
        L.check(self._lib.vdb_ivf_info(self._h, C.byref(p), C.byref(k), C.byref(d)))
        return {"present": bool(p.value), "k": int(k.value), "default_n_probes": int(d.value)}

    def has_ivf(self) -> bool:
        return self.ivf_info()["present"]

    def ivf_export(self):
        info = self.ivf_info()
        cent = np.zeros((info["k"], self.dim), dtype=np.float32)
        assign = np.zeros(len(self), dtype=np.uint64)
        L.check(self._lib.vdb_ivf_export(self._h, _ptr(cent, L.f32p), _ptr(assign, L.u64p)))
        return {"centroids": cent, "assign": assign}

    def ivf_knn(self, queries, k: int, n_probes: int = 0):
        """IVFIndex::knn_with_ef (ef = n_probes; 0 -> default 4)."""
        return self._knn_call(self._lib.vdb_ivf_knn, queries, k, int(n_probes))

    def ivf_knn_device(self, q_ptr: int, nq: int, k: int, n_probes: int, out_idx_ptr: int, out_dist_ptr: int,
                       out_cnt_ptr: int, stream: int = 0):
        L.check(self._lib.vdb_ivf_knn_device(self._h, L.vp(q_ptr), int(nq), self.dim, int(k), int(n_probes),
                                             L.vp(out_idx_ptr), L.vp(out_dist_ptr), L.vp(out_cnt_ptr), L.vp(stream)))

    # -- measurement ---------------------------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        L.check(self._lib.vdb_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        L.check(self._lib.vdb_prof_reset(self._h))

    def prof_get(self, kernel: str):
        ms, n, by = C.c_double(), C.c_uint64(), C.c_double()
        L.check(self._lib.vdb_prof_get(self._h, kernel.encode(), C.byref(ms), C.byref(n), C.byref(by)))
        return {"ms": float(ms.value), "launches": int(n.value), "bytes": float(by.value)}


def stream_probe(device: int = 0, nbytes: int = 3_840_000_000, iters: int = 5) -> float:
    """Attainable HBM read bandwidth of this box in GB/s: pure streaming read, best of two patterns."""
    v = C.c_double()
    L.check(L.load().vdb_stream_probe(int(device), int(nbytes), int(iters), C.byref(v)))
    return float(v.value)


def stream_probe_rows(device: int = 0, nbytes: int = 1_920_000_000, iters: int = 5, row_bytes: int = 1920) -> float:
    """GB/s of MFMA A-fragment loads (16 rows x 64 B per instruction) from a row-major image of rows of row_bytes (multiple of 128; 1920 = a 960-d fp16 row)."""
    v = C.c_double()
    L.check(L.load().vdb_stream_probe_rows(int(device), int(nbytes), int(iters), int(row_bytes), C.byref(v)))
    return float(v.value)


def mfma_probe(device: int = 0, waves_per_simd: int = 2, iters: int = 200_000, i8: bool = False):
    """(dense fp16 TFLOP/s, shader clock in GHz) of back-to-back v_mfma_f32_16x16x32_f16 on every SIMD of this box;
    i8=True: (dense int8 TOP/s, clock) of v_mfma_i32_16x16x64_i8, the 8-bit Flat filter's instruction."""
    t, c = C.c_double(), C.c_double()
    fn = L.load().vdb_mfma_probe_i8 if i8 else L.load().vdb_mfma_probe
    L.check(fn(int(device), int(waves_per_simd), int(iters), C.byref(t), C.byref(c)))
    return float(t.value), float(c.value)


def latency_probe(device: int = 0, nbytes: int = 1 << 30, hops: int = 20000) -> float:
    """Nanoseconds per DEPENDENT HBM load on this box (one lane chasing a random cycle over 128-B lines of an nbytes buffer)."""
    v = C.c_double()
    L.check(L.load().vdb_latency_probe(int(device), int(nbytes), int(hops), C.byref(v)))
    return float(v.value)


def fold_probe(device: int = 0, adds: int = 1 << 22) -> float:
    """Nanoseconds per DEPENDENT f32 add on this box (the chain a strict left fold is made of)."""
    v = C.c_double()
    L.check(L.load().vdb_fold_probe(int(device), int(adds), C.byref(v)))
    return float(v.value)


def remove_plan(n: int, rows):
    """(dst, src) of vdb_remove_plan: the moves that removing the strictly ascending `rows` from a table of n rows comes to -- the net
    effect of swap_remove on them in descending order.  Pure host code; an unsorted, duplicate or out-of-range list raises VdbError."""
    r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
    dst = np.zeros(r.size, dtype=np.uint64)
    src = np.zeros(r.size, dtype=np.uint64)
    moves = C.c_uint64()
    L.check(L.load().vdb_remove_plan(int(n), _ptr(r, L.u64p), r.size, _ptr(dst, L.u64p), _ptr(src, L.u64p), C.byref(moves)))
    return dst[:int(moves.value)].copy(), src[:int(moves.value)].copy()


def merge_topk(dists: np.ndarray, ids: np.ndarray, counts: np.ndarray, k: int):
    """Merge per-shard sorted lists [S][nq][k] into the global top-k by (distance, index)."""
    d = _f32(dists)
    i = np.ascontiguousarray(ids, dtype=np.uint64)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    S, nq = d.shape[0], d.shape[1]
    oi = np.zeros((nq, k), dtype=np.uint64)
    od = np.zeros((nq, k), dtype=np.float32)
    oc = np.zeros(nq, dtype=np.uint64)
    L.check(L.load().vdb_merge_topk(_ptr(d, L.f32p), _ptr(i, L.u64p), _ptr(c, L.u64p), S, nq, k, _ptr(oi, L.u64p),
                                    _ptr(od, L.f32p), _ptr(oc, L.u64p)))
    return oi, od, oc


def range_merge(lims, ids, dists, limit: int | None = None):
    """Merge per-shard range results (vdb_range_merge, host utility): `lims` [S][nq + 1] CSR offsets of every shard (each row from
    0), `ids` / `dists` either [S][stride] arrays (shard s's pairs at the front of row s) or sequences of S arrays of lims[s][nq]
    pairs.  Returns (lims, idx, dist) like GpuIndex.range_search: per query the union ascending by (distance, id), the first
    `limit` of it when given."""
    if limit is not None and int(limit) <= 0:
        raise ValueError("limit must be positive (None: no limit)")
    lm = np.ascontiguousarray(lims, dtype=np.uint64)
    if lm.ndim != 2 or lm.shape[1] < 1:
        raise ValueError("lims must be [S][nq + 1]")
    S, nq = lm.shape[0], lm.shape[1] - 1
    if isinstance(ids, np.ndarray) and ids.ndim == 2:
        i = np.ascontiguousarray(ids, dtype=np.uint64)
        d = _f32(dists)
    else:
        stride = max([len(x) for x in ids] + [1])
        i = np.zeros((S, stride), dtype=np.uint64)
        d = np.zeros((S, stride), dtype=np.float32)
        for s in range(S):
            i[s, :len(ids[s])] = ids[s]
            d[s, :len(dists[s])] = dists[s]
    if i.shape != d.shape or i.shape[0] != S:
        raise ValueError("ids and dists must hold one row of pairs per shard")
    lib = L.load()
    ol = np.zeros(nq + 1, dtype=np.uint64)
    L.check(lib.vdb_range_merge(_ptr(lm, L.u64p), None, None, S, nq, i.shape[1], int(limit or 0), _ptr(ol, L.u64p), None, None))
    oi = np.zeros(int(ol[nq]), dtype=np.uint64)
    od = np.zeros(int(ol[nq]), dtype=np.float32)
    L.check(lib.vdb_range_merge(_ptr(lm, L.u64p), _ptr(i, L.u64p), _ptr(d, L.f32p), S, nq, i.shape[1], int(limit or 0), _ptr(ol, L.u64p),
                                _ptr(oi, L.u64p), _ptr(od, L.f32p)))
    return ol, oi, od


def pq_merge_resort(adc_keys: np.ndarray, exact_keys: np.ndarray, k: int):
    """Merge per-shard ADC shortlists [S][nq][efk] (pair keys, see vdbhip.h) and replay pq_resort."""
    a = np.ascontiguousarray(adc_keys, dtype=np.uint64)
    e = np.ascontiguousarray(exact_keys, dtype=np.uint64)
    S, nq, efk = a.shape
    oi = np.zeros((nq, k), dtype=np.uint64)
    od = np.zeros((nq, k), dtype=np.float32)
    oc = np.zeros(nq, dtype=np.uint64)
    L.check(L.load().vdb_pq_merge_resort(_ptr(a, L.u64p), _ptr(e, L.u64p), S, nq, efk, k, _ptr(oi, L.u64p),
                                         _ptr(od, L.f32p), _ptr(oc, L.u64p)))
    return oi, od, oc
