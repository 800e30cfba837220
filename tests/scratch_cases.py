"""The case table of tests/test_scratch_poison_gpu.py and tests/test_call_history_gpu.py: one row per entry point of GpuIndex -- a name, the
table it runs on, a closure that makes the call with fixed seeded arguments, the get_stat counters that prove which route answered, and
(where tests/ or oracle has one) a CPU reference of the answer.

Every read-side call of an index takes the same pooled Workspace when one thread calls; its buffers are shared by every feature and are
neither cleared nor shrunk between calls.  The invariant the two files state: THE BITS A CALL RETURNS, AND THE ROUTE IT TOOK, DO NOT DEPEND ON
WHAT ITS SCRATCH HELD BEFORE.  A row's baseline is its answer on an index that has made no other call (run twice: it must repeat bit for
bit), checked against the CPU reference so that two equal wrong answers do not pass.

Every closure pins the routing parameters first (Env.route): the automatic modes follow the redo rates of earlier calls by design, so a
forced route is what makes "the route it took" comparable across histories.  flat_i8_refine is pinned off (1), and on (2) in one row: its
automatic state counts calls.

Tables: f32 22 037 x 128 (= 16 * 1377 + 5 = 192 * 114 + 149: ragged last tiles, two 64-wide k blocks so that the 8-bit and fp16 filters can
be forced) under L2Sqr and Cosine, f32 1003 x 128 (small-table paths; rows 900 .. 939 sit within 0.05 of row 7: the dense spot of the
self-join rows), u8 20 003 x 128.  Two label columns on the f32 tables: 0 = row % 5 (row % 11 == 0: none), 1 = row // 4 % 50 (row % 13 == 0: none).
Queries: rows of the table plus noise; query 5 of each set has a NaN coordinate (the hand-on / redo path).  The rescoring rows take their
candidates from the oracle's lists and score whole groups of label column 1 (tests/rescore_ref.py)."""
import numpy as np

import dbscan_ref
import dup_ref
import fuse_groups_ref
import fuse_ref
import like_ref
import lof_ref
import mmr_ref
import rescore_ref

DIM, N_BIG, N_SMALL, N_U8 = 128, 22037, 1003, 20003
NONE = 0xFFFFFFFF
PATTERNS = (0x00000001, 0xFFFFFFFF, 0x7F800000)  # a small count / id / denormal | LABEL_NONE, PAIR_NONE, a NaN | +inf as a key

# every cumulative counter of vdb_get_stat (high-water marks, "last call" values and validity flags are no deltas and stay out)
COUNTERS = (
    "flat_fallback", "flat_half_queries", "flat_half_redo", "flat_i8_queries", "flat_i8_redo", "flat_u8_queries", "flat_u8_redo",
    "flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits", "flat_range_results", "flat_filtered_queries",
    "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries", "flat_filtered_multi_calls",
    "flat_filtered_grouped_queries", "flat_range_multi_calls", "flat_range_grouped_queries", "mirror_alloc_failures", "flat_i8_second_queries",
    "flat_i8_second_redo", "flat_i8_refine_queries", "pq_adc16_queries", "pq_adc16_redo", "pq_q8_overflow", "pq_q8_short", "pq_q8_hits_sum",
    "mask_where_masks", "mask_where_set_masks", "mask_where_any_masks", "mask_combine_masks", "mask_partition_masks", "label_count_calls",
    "label_lookup_calls", "label_lookup_codes", "label_lookup_direct", "label_lookup_passes", "kmeans_calls", "kmeans_iterations",
    "kmeans_rows_assigned", "kmeans_unsure_rows", "flat_dup_calls", "flat_dup_chunks", "flat_dup_pairs", "flat_dbscan_calls", "flat_dbscan_chunks",
    "flat_dbscan_pairs", "flat_knn_graph_calls", "flat_knn_graph_chunks", "pca_cov_calls", "pca_cov_rows", "pca_project_calls", "pca_project_rows",
    "silhouette_calls", "silhouette_rows", "flat_grouped_calls", "flat_grouped_queries", "flat_grouped_rounds", "flat_grouped_exhausted_queries",
    "flat_vote_queries", "flat_vote_scratch", "flat_mmr_calls", "flat_mmr_queries", "flat_like_calls", "flat_like_queries", "like_example_rows",
    "flat_fused_calls", "flat_fused_queries", "flat_fused_lists", "flat_fused_groups_calls", "flat_fused_groups_queries", "flat_fused_groups_lists",
    "flat_rescore_calls", "flat_rescore_questions", "flat_rescore_rows",
    "update_calls", "update_rows", "fetch_calls", "fetch_rows", "fetch_chunks", "fetch_direct", "labels_scatter_calls", "labels_scatter_rows",
)
ROUTE_DEFAULTS = {"flat_small": 0, "flat_half": 0, "flat_i8": 0, "flat_u8": 0, "flat_filtered_direct_max": 8192, "flat_i8_refine": 1,
                  "flat_dup_chunk": 16384, "fetch_chunk_bytes": 128 << 20}


def O():
    from oracle import oracle
    return oracle


class Data:
    """the tables, labels and queries, made once"""

    def __init__(self):
        rng = np.random.default_rng(1806)
        off = (rng.standard_normal(DIM) * 0.5).astype(np.float32)
        self.big = rng.standard_normal((N_BIG, DIM)).astype(np.float32) + off
        self.small = rng.standard_normal((N_SMALL, DIM)).astype(np.float32) + off
        self.small[900:940] = self.small[7] + rng.standard_normal((40, DIM)).astype(np.float32) * np.float32(0.01)
        self.u8 = rng.integers(0, 256, (N_U8, DIM), dtype=np.uint8)
        rows = np.arange(N_BIG)
        self.lab0 = np.where(rows % 11 == 0, NONE, rows % 5).astype(np.uint32)
        self.lab1 = np.where(rows % 13 == 0, NONE, rows // 4 % 50).astype(np.uint32)
        self.allow_a, self.allow_b = rows % 3 == 0, rows < 6000
        self.q_big = self.big[rng.permutation(N_BIG)[:150]] + rng.standard_normal((150, DIM)).astype(np.float32) * np.float32(0.05)
        self.q_small = self.small[rng.permutation(N_SMALL)[:150]] + rng.standard_normal((150, DIM)).astype(np.float32) * np.float32(0.05)
        # integer-valued, so that every distance to a u8 row is an exact integer below 2^24 in any summation order
        self.q_u8 = np.clip(self.u8[rng.permutation(N_U8)[:150]].astype(np.float32) + rng.integers(-3, 4, (150, DIM)), 0, 255).astype(np.float32)
        for q in (self.q_big, self.q_small, self.q_u8):
            q[5, 3] = np.nan
        self.perm = rng.permutation(N_BIG)[:500]
        self.upd_vecs = rng.standard_normal((3, DIM)).astype(np.float32) + off
        self.W = rng.standard_normal((2, DIM)).astype(np.float32)
        self._memo = {}
        self._ann = None

    def rows_of(self, kind):
        return {"big_l2": self.big, "big_cos": self.big, "small": self.small, "ann": self.small, "hnsw": self.small,
                "u8": self.u8.astype(np.float32)}[kind]

    def queries_of(self, kind):
        return {"big_l2": self.q_big, "big_cos": self.q_big, "u8": self.q_u8}.get(kind, self.q_small)

    def order(self, kind, q0, q1, k):
        """the oracle's first k (ids, distances) of queries [q0, q1) of the kind's query set, remembered"""
        key = (kind, q0, q1, k)
        if key not in self._memo:
            met = O().COSINE if kind == "big_cos" else O().L2SQR
            self._memo[key] = O().flat_knn_batch(self.rows_of(kind), self.queries_of(kind)[q0:q1], k, met, nthreads=16)[:2]
        return self._memo[key]

    def self_order(self):
        """every row of the small table against all of it, in the oracle's order"""
        if "self" not in self._memo:
            self._memo["self"] = O().flat_knn_batch(self.small, self.small, N_SMALL, O().L2SQR, nthreads=16)[:2]
        return self._memo["self"]

    def radii(self, kind, q0, q1, rank):
        return self.order(kind, q0, q1, 256)[1][:, rank].copy()

    def ann(self, vdb):
        """PQ, IVF and HNSW structures over the small table, built ONCE on an index of their own and exported: the rows attach them, so
        that a builder's nondeterminism plays no part"""
        if self._ann is None:
            ix = vdb.GpuIndex(DIM, "l2sqr")
            ix.batch_add(self.small)
            ix.pq_build(n_bits=4, m=32, train_n=500, max_iter=5, seed=7)
            ix.ivf_build(16, max_iter=5, seed=42)
            ix.hnsw_build(M=16, ef_construction=100, seed=42, batch=1, nthreads=1)
            self._ann = {"pq": ix.pq_export(), "ivf": ix.ivf_export(), "hnsw": ix.hnsw_export()}
            ix.close()
        return self._ann


_DATA = None


def data():
    global _DATA
    if _DATA is None:
        _DATA = Data()
    return _DATA


class Env:
    """one index of a kind with its labels, its host-made masks and (ann, hnsw) its attached structures"""

    def __init__(self, vdb, kind):
        D = data()
        self.vdb, self.D, self.kind = vdb, D, kind
        self.q = D.queries_of(kind)
        if kind == "edit":
            self.ix = None
            return
        if kind == "u8":
            self.ix = vdb.GpuIndex(DIM, "l2sqr", scalar="u8")
            self.ix.batch_add_u8(D.u8)
        else:
            rows = D.rows_of(kind)
            self.ix = vdb.GpuIndex(DIM, "cosine" if kind == "big_cos" else "l2sqr")
            self.ix.batch_add(rows)
            self.ix.set_labels(0, D.lab0[:len(rows)])
            self.ix.set_labels(1, D.lab1[:len(rows)])
        self.n = len(self.ix)
        if kind in ("ann", "hnsw"):
            a = D.ann(vdb)
            self.ix.pq_attach(4, 32, a["pq"]["centroids"], a["pq"]["codes"])
            if kind == "ann":
                self.ix.ivf_attach(a["ivf"]["centroids"], a["ivf"]["assign"])
            else:
                self.ix.hnsw_attach(16, 100, a["hnsw"])
        self._masks = {}

    def mask(self, name):
        if name not in self._masks:
            allow = {"a": self.D.allow_a, "b": self.D.allow_b}[name][:self.n]
            self._masks[name] = self.ix.make_mask(allow)
        return self._masks[name]

    def route(self, mode=0, **params):
        self.ix.set_flat_mode(mode)
        for name, value in {**ROUTE_DEFAULTS, **params}.items():
            self.ix.set_param(name, value)

    def snap(self):
        return [] if self.ix is None else [self.ix.get_stat(s) for s in COUNTERS]

    def close(self):
        if self.ix is not None:
            for m in self._masks.values():
                m.close()
            self.ix.close()
            self.ix = None


class Case:
    """route: counters that must move in the baseline; still: counters that must NOT; prof: {kernel name: launches} of one more baseline
    run with the profiling hooks on (the proof of a route that has no counter)"""

    def __init__(self, name, kind, fn, route=(), ref=None, family=None, still=(), prof=None):
        self.name, self.kind, self.fn, self.route, self.ref = name, kind, fn, tuple(route), ref
        self.family, self.still, self.prof = family or name.split("-")[0], tuple(still), prof

    def run(self, env):
        """(result, counter deltas)"""
        before = env.snap()
        got = self.fn(env)
        return got, [a - b for a, b in zip(env.snap(), before)]


def same(a, b):
    """bit for bit: arrays by their bytes, except that a float NaN matches a NaN at the same position"""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if a.dtype.kind == "f":
            u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
        return bool(np.array_equal(a, b))
    if isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b):
        return True
    return type(a) is type(b) and a == b


def moved(case, deltas):
    return {s: deltas[COUNTERS.index(s)] for s in case.route}


# ---- the CPU references ---------------------------------------------------------------------------------------------------------------------
def _lists_equal(got, oi, od, what):
    """idx / dist / cnt [nq][k] of a k-NN answer == the oracle's lists (distances of a NaN query: NaN by position)"""
    idx, dist, cnt = got[:3]
    k = idx.shape[1]
    assert (cnt == k).all(), what
    assert np.array_equal(idx, oi[:, :k]) and same(dist, np.ascontiguousarray(od[:, :k])), (what, np.flatnonzero((idx != oi[:, :k]).any(1))[:8])


def ref_knn(q0, q1, k):
    def check(env, got):
        _lists_equal(got, *env.D.order(env.kind, q0, q1, k), "flat_knn")
    return check


def _range_lists(oi, od, radii, allow=None):
    out = []
    for q in range(len(oi)):
        keep = od[q] <= radii[q]
        assert keep.sum() < len(od[q]), "the oracle's list must reach past the radius"
        if allow is not None:
            keep &= allow[q][oi[q].astype(np.int64)]
        out.append((oi[q][keep], od[q][keep]))
    return out


def _range_equal(got, lists):
    lims, idx, dist = got
    assert lims.tolist() == np.concatenate([[0], np.cumsum([len(i) for i, _ in lists])]).tolist()
    assert np.array_equal(idx, np.concatenate([i for i, _ in lists])) and same(dist, np.concatenate([d for _, d in lists]))


def ref_range(q0, q1, rank, masks_of=None):
    def check(env, got):
        oi, od = env.D.order(env.kind, q0, q1, 256)
        allow = None if masks_of is None else [{"a": env.D.allow_a, "b": env.D.allow_b}[m][:env.n] for m in masks_of]
        _range_equal(got, _range_lists(oi, od, env.D.radii(env.kind, q0, q1, rank), allow))
    return check


def ref_filtered(q0, q1, k, masks_of):
    def check(env, got):
        oi, od = env.D.order(env.kind, q0, q1, 256)
        idx, dist, cnt = got
        for q in range(q1 - q0):
            keep = {"a": env.D.allow_a, "b": env.D.allow_b}[masks_of[q]][oi[q].astype(np.int64)]
            assert keep.sum() >= k and cnt[q] == k
            assert np.array_equal(idx[q], oi[q][keep][:k]) and same(dist[q], np.ascontiguousarray(od[q][keep][:k])), q
    return check


def ref_mmr(q0, q1, k, fetch_k, lam):
    def check(env, got):
        oi, od = env.D.order(env.kind, q0, q1, fetch_k)
        rd = mmr_ref.RowDist(env.D.rows_of(env.kind), O().L2SQR)
        want = mmr_ref.expect(rd, oi, od, np.full(q1 - q0, fetch_k), k, lam)
        assert same(tuple(got), tuple(want)), "mmr"
    return check


def ref_like(pos, neg, k):
    def check(env, got):
        rows = env.D.rows_of(env.kind)
        qs = like_ref.like_queries(rows, pos, neg)
        oi, od, _ = O().flat_knn_batch(rows, qs, 64, O().L2SQR)
        idx, dist, cnt = got
        for q in range(len(pos)):
            keep = like_ref.drop_listed(oi[q], list(pos[q]) + list(neg[q]), k)
            assert cnt[q] == k and np.array_equal(idx[q], oi[q][keep]) and same(dist[q], np.ascontiguousarray(od[q][keep])), q
    return check


def _fused_equal(got, q, ids, scores):
    idx, dist, cnt = got[:3]
    assert cnt[q] == len(ids) and np.array_equal(idx[q, :len(ids)], ids) and same(dist[q, :len(ids)].copy(), scores), q


def ref_fused(q0, lims, k, fetch_k, mode):
    def check(env, got):
        oi, od = env.D.order(env.kind, q0, q0 + lims[-1], fetch_k)
        for q in range(len(lims) - 1):
            _fused_equal(got, q, *fuse_ref.fuse([(oi[s], od[s]) for s in range(lims[q], lims[q + 1])], k, mode))
    return check


def ref_fused_groups(q0, lims, k, fetch_k, column, mode):
    def check(env, got):
        oi, od = env.D.order(env.kind, q0, q0 + lims[-1], fetch_k)
        group_of = fuse_groups_ref.label_groups((env.D.lab0, env.D.lab1)[column])
        for q in range(len(lims) - 1):
            ids, scores, exact = fuse_groups_ref.fuse_groups([(oi[s], od[s]) for s in range(lims[q], lims[q + 1])], group_of, k, mode, trunc_len=fetch_k)
            _fused_equal(got, q, ids, scores)
            assert int(got[3][q]) == exact, q
    return check


RESCORE_LD, RESCORE_MASK_OF = 16, [0, 1, 1, 0, 1, 0, 0, 1]


def rescore_cands(env, q0, lims):
    """the candidates of the rescoring rows: question q takes the oracle's first 5 rows of each of its sub-queries, list after list (so
    10, 15 and 15 of ld = 16; neighbours share label codes and lists share rows: duplicates of both kinds) -> (ids [nq][16], counts)"""
    oi = env.D.order(env.kind, q0, q0 + lims[-1], 12)[0]
    cand, cnt = np.zeros((len(lims) - 1, RESCORE_LD), dtype=np.uint64), np.zeros(len(lims) - 1, dtype=np.uint64)
    for q in range(len(lims) - 1):
        ids = np.concatenate([oi[s][:5] for s in range(lims[q], lims[q + 1])])
        cand[q, :len(ids)], cnt[q] = ids, len(ids)
    return cand, cnt


def ref_rescore(q0, lims, k, column, mode, masked=False):
    def check(env, got):
        nsub = lims[-1]
        key = ("rescore-dm", env.kind, q0, nsub)
        if key not in env.D._memo:  # the dense distance table of the sub-queries, from the oracle's order at k = n
            oi, od = env.D.order(env.kind, q0, q0 + nsub, env.n)
            dm = np.zeros((nsub, env.n), np.float32)
            np.put_along_axis(dm, oi.astype(np.int64), od, axis=1)
            env.D._memo[key] = dm
        cand, cnt = rescore_cands(env, q0, lims)
        allows = [env.D.allow_a[:env.n], env.D.allow_b[:env.n]] if masked else None
        idx, bits, count, _rows = rescore_ref.expect(env.D._memo[key], (env.D.lab0, env.D.lab1)[column][:env.n], lims, cand, cnt, k, mode,
                                                     allows=allows, mask_of=RESCORE_MASK_OF if masked else None)
        assert np.array_equal(got[2], count) and np.array_equal(got[0], idx) and same(got[1], bits.view(np.float32)), "rescore"
    return check


def _self_lists(env, radius):
    oi, od = env.D.self_order()
    return [[(int(i), d) for i, d in zip(oi[r][od[r] <= radius], od[r][od[r] <= radius])] for r in range(N_SMALL)]


def ref_dups(radius):
    def check(env, got):
        lims, ids = dup_ref.csr([[i for i, _ in x] for x in _self_lists(env, radius)])
        group, stats = dup_ref.dup_ref(N_SMALL, list(range(N_SMALL)), lims, ids)
        assert np.array_equal(got[0], group) and got[1] == stats, (got[1], stats)
    return check


def ref_dbscan(eps, min_samples):
    def check(env, got):
        dbscan_ref.same(got, dbscan_ref.dbscan_ref(N_SMALL, list(range(N_SMALL)), *dbscan_ref.csr(_self_lists(env, eps)), min_samples))
    return check


def ref_lof(k):
    def check(env, got):
        _, nbr, nd, cnt = lof_ref.graph_of_order(*env.D.self_order(), k)
        kdist, lrd, lof = lof_ref.of_lists(nbr, nd, cnt)
        assert same(got[0], kdist)
        lof_ref.close(got[1], lrd)
        lof_ref.close(got[2], lof)
    return check


# ---- the closures ---------------------------------------------------------------------------------------------------------------------------
TIER_COUNTERS = ("flat_half_queries", "flat_i8_queries", "flat_u8_queries")
FLAT_ROUTES = {  # name -> (kind, flat_mode, parameters, counters that must move, query counts, launches of a profiled run)
    # k_flat_small, one launch: it takes calls of at most 64 queries (flat_small_supported, k_small.hip), so 150 queries cannot reach it
    # and the row does not exist; the route has no counter, so the baseline proves it with the profiling hooks
    "small": ("small", 0, {"flat_small": 2}, (), (1, 48), {"flat_small": 1, "flat_exact": 0}),
    "scan": ("big_l2", 1, {}, (), (1, 48, 150), None),  # the many-queries strict-order scan
    "bf16": ("big_l2", 2, {"flat_i8": 1, "flat_half": 1}, (), (1, 48, 150), None),
    "fp16": ("big_l2", 2, {"flat_i8": 1, "flat_half": 2}, ("flat_half_queries",), (1, 48, 150), None),
    "i8": ("big_l2", 2, {"flat_i8": 2}, ("flat_i8_queries",), (1, 48, 150), None),
    "u8": ("u8", 0, {"flat_u8": 2}, ("flat_u8_queries",), (1, 48, 150), None),
}


def _knn(mode, params, nq, k):
    def fn(e):
        e.route(mode, **params)
        return e.ix.flat_knn(e.q[:nq], k)
    return fn


def fuse_lists_device(e, ids):
    """the fusion alone over the oracle's lists of queries 8 .. 15 with the ids given (3 fused queries of 2 / 3 / 3 lists of 12): its id
    check (ids_ok with the flag inside the upload) reads a word of grp_aux back; an id that is no row is refused AFTER that device work"""
    import torch
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).astype(np.int64)).cuda()
    d_dist = torch.from_numpy(e.D.order(e.kind, 8, 16, 12)[1]).cuda()
    d_cnt = torch.full((8,), 12, dtype=torch.int64, device="cuda")
    o_idx, o_cnt = torch.zeros((3, 5), dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda")
    o_dist = torch.zeros((3, 5), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ix.fuse_lists_device(d_ids.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), [0, 2, 5, 8], 12, 5, o_idx.data_ptr(), o_dist.data_ptr(),
                           o_cnt.data_ptr(), "rrf")
    return o_idx.cpu().numpy().view(np.uint64), o_dist.cpu().numpy(), o_cnt.cpu().numpy().view(np.uint64)


def get_rows_device(e, ids):
    """the device form of the row fetch: its id check (ids_ok) reads a flag word of ws.flags back; an id that is no row is refused after it"""
    import torch
    d_ids = torch.from_numpy(np.ascontiguousarray(ids).astype(np.int64)).cuda()
    out = torch.empty((len(ids), DIM), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e.ix.get_rows_device(d_ids.data_ptr(), len(ids), out.data_ptr())
    return out.cpu().numpy()


def _masks_rows(masks):
    out = tuple((len(m),) + tuple(m.rows()) for m in masks)
    for m in masks:
        m.close()
    return out


def _edit(tier):
    i8, half = {"i8": (2, 0), "fp16": (1, 2), "bf16": (1, 1)}[tier]

    def fn(e):
        """a disposable index: rows added past the old extent, a block removed across the new end, rows updated in place -- each edit
        followed by a search on the forced tier; the mirrors' padding and ragged tiles are allocated and re-tiled inside the call"""
        D = e.D
        ix = e.vdb.GpuIndex(DIM, "l2sqr")
        try:
            ix.batch_add(D.big[:20000])
            ix.set_flat_mode(2)
            for name, value in (("flat_i8", i8), ("flat_half", half), ("flat_i8_refine", 1)):
                ix.set_param(name, value)
            out = [ix.flat_knn(D.q_big[:48], 7)]
            ix.batch_add(D.big[20000:])
            out.append(ix.flat_knn(D.q_big[:48], 7))
            ix.remove_rows(np.arange(19036, 21037))
            out.append(ix.flat_knn(D.q_big[:48], 7))
            ix.update_rows(np.array([5, 20035, 777]), D.upd_vecs)
            out.append(ix.flat_knn(np.concatenate([D.upd_vecs, D.q_big[:45]]), 7))
            assert out[3][0][:3, 0].tolist() == [5, 20035, 777]
            return tuple(out) + ([ix.get_stat(s) for s in COUNTERS],)
        finally:
            ix.close()
    return fn


def _build_cases():
    T = []

    def add(*a, **kw):
        T.append(Case(*a, **kw))

    # Flat k-NN on every route: 1, 48 (one partial group of 128) and 150 queries (a full group + padding queries), k = 1 and 10; a route
    # below the tiers (small, scan, bf16) moves no tier counter
    for r, (kind, mode, params, route, nqs, prof) in FLAT_ROUTES.items():
        for nq in nqs:
            for k in (1, 10):
                add(f"knn-{r}-nq{nq}-k{k}", kind, _knn(mode, params, nq, k), route, ref_knn(0, nq, k), family="knn-" + r,
                    still=TIER_COUNTERS if r in ("small", "scan", "bf16") else (), prof=prof)
    add("knn-i8-refine", "big_l2", _knn(2, {"flat_i8": 2, "flat_i8_refine": 2}, 150, 10), ("flat_i8_queries", "flat_i8_refine_queries"),
        ref_knn(0, 150, 10), family="knn-i8")  # (the refinement takes calls of at least 64 queries)
    for r in ("bf16", "fp16", "i8"):
        _, mode, params, route = FLAT_ROUTES[r][:4]
        add(f"knn-cos-{r}", "big_cos", _knn(mode, params, 48, 10), route, ref_knn(0, 48, 10), family="knn-" + r,
            still=TIER_COUNTERS if r == "bf16" else ())

    # range search: the 8-bit tier, the small table's scan, one mask per query
    def rng_i8(e):
        e.route(2)
        return e.ix.range_search(e.q[8:40], e.D.radii(e.kind, 8, 40, 19))
    add("range-i8", "big_l2", rng_i8, ("flat_range_i8_queries",), ref_range(8, 40, 19))

    def rng_small(e):
        e.route(0)
        return e.ix.range_search(e.q[8:40], e.D.radii(e.kind, 8, 40, 19))
    add("range-small", "small", rng_small, ("flat_range_scan_queries",), ref_range(8, 40, 19))
    add("range-u8", "u8", rng_small, ("flat_range_queries",), ref_range(8, 40, 19))
    MASK_OF = [0, 1, 1, 0, 1, 0, 0, 1, 1]

    def rng_multi(e):
        e.route(2)
        return e.ix.range_search_multi(e.q[8:17], e.D.radii(e.kind, 8, 17, 59), [e.mask("a"), e.mask("b")], MASK_OF)
    add("range-multi", "big_l2", rng_multi, ("flat_range_multi_calls",), ref_range(8, 17, 59, ["ab"[m] for m in MASK_OF]))

    # filtered k-NN: the gathered direct path, the 8-bit pass with the masked row constants, one mask per query
    def filt(direct_max):
        def fn(e):
            e.route(2, flat_filtered_direct_max=direct_max)
            return e.ix.flat_knn_filtered(e.q[8:40], 10, e.mask("a"))
        return fn
    add("filtered-direct", "big_l2", filt(8192), ("flat_filtered_direct_queries",), ref_filtered(8, 40, 10, "a" * 32))
    add("filtered-i8", "big_l2", filt(0), ("flat_filtered_i8_queries",), ref_filtered(8, 40, 10, "a" * 32))

    def filt_multi(e):
        e.route(2)
        return e.ix.flat_knn_filtered_multi(e.q[8:17], 10, [e.mask("a"), e.mask("b")], MASK_OF)
    add("filtered-multi", "big_l2", filt_multi, ("flat_filtered_grouped_queries",), ref_filtered(8, 17, 10, ["ab"[m] for m in MASK_OF]))

    # the list re-rankers, over lists of the 8-bit tier
    def rerank(call):
        def fn(e):
            e.route(2, flat_i8=2)
            return call(e)
        return fn
    LIMS, POS, NEG = [0, 2, 5, 8], [[1, 2], [7], [100, 200, 300]], [[5], [], [9]]
    add("grouped", "big_l2", rerank(lambda e: e.ix.flat_knn_grouped(e.q[8:24], 5, 0, 1)), ("flat_grouped_queries",))
    add("mmr", "big_l2", rerank(lambda e: e.ix.flat_knn_mmr(e.q[8:16], 4, 12, 0.5)), ("flat_mmr_queries",), ref_mmr(8, 16, 4, 12, 0.5))
    add("like", "big_l2", rerank(lambda e: e.ix.flat_knn_like(POS, 10, NEG)), ("flat_like_queries",), ref_like(POS, NEG, 10))
    add("fused-rrf", "big_l2", rerank(lambda e: e.ix.flat_knn_fused(e.q[8:16], LIMS, 5, 12, "rrf")), ("flat_fused_lists",),
        ref_fused(8, LIMS, 5, 12, "rrf"), family="fused")
    add("fused-min", "big_l2", rerank(lambda e: e.ix.flat_knn_fused(e.q[8:16], LIMS, 5, 12, "min")), ("flat_fused_lists",),
        ref_fused(8, LIMS, 5, 12, "min"), family="fused")
    # the exact rescoring borrows grp_aux, grp_ids, grp_dist, grp_cnt, grp_table, grp_q, lists, dense and qsq; it leaves tslot uncleared and
    # its entry lists rely on a padding fill.  Over label column 1: 50 codes of about 400 rows, and unlabelled rows.  The rows stand on both
    # sides of fused_groups, which fills the same grp_* buffers with another layout: test_call_history_gpu.py takes as a row's polluter the
    # next row of another family, so rescore-sum and rescore-min run BEHIND fused_groups, and fused_groups behind rescore-masks
    def rescore(mode, masked=False):
        def fn(e):
            e.route(2, flat_i8=2)
            cand, cnt = rescore_cands(e, 8, LIMS)
            kw = {"masks": [e.mask("a"), e.mask("b")], "mask_of": RESCORE_MASK_OF} if masked else {}
            return e.ix.rescore_groups(e.q[8:16], LIMS, cand, cnt, 5, 1, mode, **kw)
        return fn
    for kind, tag in (("big_l2", ""), ("big_cos", "cos-")):
        add(f"rescore-{tag}sum", kind, rescore("sum"), ("flat_rescore_rows",), ref_rescore(8, LIMS, 5, 1, "sum"))
        add(f"rescore-{tag}min", kind, rescore("min"), ("flat_rescore_rows",), ref_rescore(8, LIMS, 5, 1, "min"))
    add("fused_groups", "big_l2", rerank(lambda e: e.ix.flat_knn_fused_groups(e.q[8:16], LIMS, 5, 12, 1, "sum", return_exact=True)),
        ("flat_fused_groups_lists",), ref_fused_groups(8, LIMS, 5, 12, 1, "sum"))
    for kind, tag in (("big_l2", ""), ("big_cos", "cos-")):
        add(f"rescore-{tag}masks", kind, rescore("sum", masked=True), ("flat_rescore_rows",), ref_rescore(8, LIMS, 5, 1, "sum", masked=True))
    add("fuse_lists_device", "big_l2", lambda e: fuse_lists_device(e, e.D.order(e.kind, 8, 16, 12)[0]), (), ref_fused(8, LIMS, 5, 12, "rrf"),
        family="fused")
    add("vote", "big_l2", rerank(lambda e: e.ix.flat_knn_vote(e.q[8:24], 9, 0, 3)), ("flat_vote_queries",))

    # masks, labels and rows
    def LT(*a, **kw):
        import lab_1806_vec_db_amd as vdb
        return vdb.LabelTerm(*a, **kw)
    add("mask_where", "big_l2", lambda e: _masks_rows([e.ix.make_mask_where([(0, 2), (1, 7)])]), ("mask_where_masks",), family="masks")
    add("mask_where_sets", "big_l2", lambda e: _masks_rows([e.ix.make_mask_where_sets([LT(0, 0, 3, codes=[0, 3]), LT(1, 10, 30, negate=True)])]),
        ("mask_where_set_masks",), family="masks")
    add("mask_where_any", "big_l2", lambda e: _masks_rows([e.ix.make_mask_where_any([[LT(0, 0, 0), LT(1, 0, 9)], [LT(0, 4, 4)]])]),
        ("mask_where_any_masks",), family="masks")
    add("masks_partition", "big_l2", lambda e: _masks_rows(e.ix.make_masks_partition(0, [2, 0, NONE, 4])), ("mask_partition_masks",), family="masks")
    add("combine_masks", "big_l2", lambda e: _masks_rows([e.ix.combine_masks("or", [e.mask("a"), e.mask("b")], [True, False])]),
        ("mask_combine_masks",), family="masks")
    add("label_counts", "big_l2", lambda e: e.ix.label_counts(0, [0, 1, 2, NONE]), ("label_count_calls",), family="labels")
    add("label_counts-mask", "big_l2", lambda e: e.ix.label_counts(0, [0, 1, 2, NONE], e.mask("b")), ("label_count_calls",), family="labels")
    add("label_lookup", "big_l2", lambda e: e.ix.label_lookup(1, [3, 49, 777, NONE]), ("label_lookup_calls",), family="labels")

    def rows_gathered(e):
        e.route(0, fetch_chunk_bytes=64 * DIM * 4)
        return e.ix.get_rows(e.D.perm)
    add("get_rows", "big_l2", rows_gathered, ("fetch_chunks",))

    def rows_ref(e, got):
        assert same(got, e.D.big[e.D.perm]), "the rows fetched are the table's"
    add("get_rows_device", "big_l2", lambda e: get_rows_device(e, e.D.perm), ("fetch_rows",), rows_ref, family="get_rows")

    # analytics, on the small table
    def small(call, **params):
        def fn(e):
            e.route(0, **params)
            return call(e)
        return fn
    add("dup_groups", "small", small(lambda e: e.ix.dup_groups(0.05), flat_dup_chunk=256), ("flat_dup_chunks",), ref_dups(0.05))
    add("dbscan", "small", small(lambda e: e.ix.dbscan(0.05, 3), flat_dup_chunk=256), ("flat_dbscan_chunks",), ref_dbscan(0.05, 3))
    add("knn_graph", "small", small(lambda e: e.ix.knn_graph(5), flat_dup_chunk=256), ("flat_knn_graph_chunks",))
    add("outliers", "small", small(lambda e: e.ix.outliers(5), flat_dup_chunk=256), ("flat_knn_graph_chunks",), ref_lof(5))
    add("covariance", "small", small(lambda e: e.ix.covariance()), ("pca_cov_rows",), family="pca")
    add("project", "small", small(lambda e: e.ix.project(e.D.W, e.D.small.astype(np.float64).mean(0))), ("pca_project_rows",), family="pca")
    add("silhouette", "small", small(lambda e: e.ix.silhouette(0)), ("silhouette_rows",), family="silhouette")
    add("silhouette-mask", "small", small(lambda e: e.ix.silhouette(0, e.mask("a"))), ("silhouette_rows",), family="silhouette")
    add("silhouette-euclid", "small", small(lambda e: e.ix.silhouette(0, euclidean=True)), ("silhouette_rows",), family="silhouette")
    add("kmeans", "small", small(lambda e: e.ix.kmeans(8, max_iter=5, seed=3, init=e.D.small[::130][:8])), ("kmeans_iterations",), family="kmeans")
    add("kmeans_assign", "small", small(lambda e: e.ix.kmeans_assign(e.D.small[::130][:8])), ("kmeans_rows_assigned",), family="kmeans")

    # ANN over attached structures
    def hnsw_walk(e):
        e.route(0)
        return tuple(e.ix.knn_with_ef(e.q[8:24], 10, 64)) + (e.ix.hnsw_last_stats(),)
    add("knn_pq", "ann", small(lambda e: e.ix.knn_pq(e.q[8:24], 10, 64)), family="ann")
    add("ivf_knn", "ann", small(lambda e: e.ix.ivf_knn(e.q[8:24], 10, 4)), family="ann")
    add("knn_with_ef", "hnsw", hnsw_walk, family="ann")
    add("knn_pq-hnsw", "hnsw", small(lambda e: e.ix.knn_pq(e.q[8:24], 10, 64)), family="ann")

    # edits on a disposable index
    for tier in ("i8", "fp16", "bf16"):
        add("edits-" + tier, "edit", _edit(tier), family="edits")
    return T


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_ENVS, _BASE = {}, {}


def shared_env(vdb, kind):
    """THE index of a kind that every case of the session shares: one thread, so one workspace serves all its calls"""
    if kind not in _ENVS:
        _ENVS[kind] = Env(vdb, kind)
    return _ENVS[kind]


def close_shared():
    """closes the shared indexes (the finaliser of each of the two files; the baselines are plain arrays and stay for the session)"""
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def baseline(vdb, case):
    """(result, counter deltas) of the case on an index that has made no other call: run twice, bit for bit the same (every row of the
    table is: none needed a tolerance), the counters of its route moved, the answer equal to the CPU reference"""
    if case.name not in _BASE:
        env = Env(vdb, case.kind)
        try:
            first, second = case.run(env), case.run(env)
            assert same(first[0], second[0]), f"{case.name}: two runs on a fresh index differ"
            assert first[1] == second[1], (case.name, [(s, a, b) for s, a, b in zip(COUNTERS, first[1], second[1]) if a != b])
            assert all(v > 0 for v in moved(case, first[1]).values()), (case.name, moved(case, first[1]))
            assert all(first[1][COUNTERS.index(s)] == 0 for s in case.still), (case.name, [first[1][COUNTERS.index(s)] for s in case.still])
            if case.ref is not None:
                case.ref(env, first[0])
            if case.prof is not None:  # (last: the hooks stay on for the rest of this index's life)
                env.ix.prof_enable(True)
                third = case.run(env)
                assert same(third[0], first[0]) and third[1] == first[1], f"{case.name}: the profiled run differs"
                launches = {kernel: env.ix.prof_get(kernel)["launches"] for kernel in case.prof}
                assert launches == case.prof, (case.name, launches)
        finally:
            env.close()
        _BASE[case.name] = first
    return _BASE[case.name]


def check(vdb, case, what=""):
    """the case on the shared index == its baseline, answer and counters"""
    want = baseline(vdb, case)
    got = case.run(shared_env(vdb, case.kind))
    assert same(got[0], want[0]), f"{case.name} {what}: the answer differs from the baseline"
    assert got[1] == want[1], (case.name, what, [(s, a, b) for s, a, b in zip(COUNTERS, got[1], want[1]) if a != b])
