"""The rule of the fused multi-query search (include/vdbhip.h, vdb_flat_knn_fused / vdb_fuse_lists_device) as a loop over np.float32
scalars: one rounding per operation, no FMA, the fold in ascending list order.  tests/test_fuse_ref_cpu.py verifies it on hand-computed
cases and against a brute-force restatement; the GPU tests compare the kernel with it bit for bit.

A list is (ids, dists): the entries that count, in rank order (the caller cuts at min(count, ld)).  Of an id that occurs more than once
in one list only the first occurrence counts."""
import numpy as np

F = np.float32
RRF, MIN = "rrf", "min"


def order_key(d) -> int:
    """the knn order of a distance as an integer: -0 == +0, every NaN equal and last (f32_orderable of csrc/common.hpp)"""
    d = F(d) + F(0.0)
    u = int(np.array(d, dtype=np.float32).view(np.uint32))
    if (u & 0x7FFFFFFF) > 0x7F800000:
        u = 0x7FC00000
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def bits(x) -> int:
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def fuse(lists, k, mode=RRF, weights=None, c=60.0):
    """-> (ids, scores): the first min(k, distinct ids) entries of the fused answer; scores as np.float32 (compare their bits)"""
    c = F(c)
    acc = {}  # id -> score so far
    with np.errstate(all="ignore"):
        for s, (ids, dists) in enumerate(lists):
            w = F(1.0) if weights is None else F(weights[s])
            seen = set()
            for p, (i, d) in enumerate(zip(ids, dists)):
                i = int(i)
                if i in seen:
                    continue
                seen.add(i)
                if mode == RRF:
                    den = F(F(p + 1) + c)
                    term = F(w / den)
                    acc[i] = F(acc.get(i, F(0.0)) + term)
                else:
                    d = F(d)
                    if i not in acc or order_key(d) < order_key(acc[i]):
                        acc[i] = d
        if mode == RRF:
            ranked = sorted(acc, key=lambda i: (order_key(-acc[i]), i))
        else:
            ranked = sorted(acc, key=lambda i: (order_key(acc[i]), i))
    ranked = ranked[:k]
    return np.array(ranked, dtype=np.uint64), np.array([acc[i] for i in ranked], dtype=np.float32)


def padded(ids, scores, k):
    """the answer as the library lays it out: [k] ids and [k] score bit patterns with zeros behind the count, and the count"""
    oi = np.zeros(k, dtype=np.uint64)
    ob = np.zeros(k, dtype=np.uint32)
    oi[:len(ids)] = ids
    ob[:len(ids)] = np.asarray(scores, dtype=np.float32).view(np.uint32)
    return oi, ob, len(ids)
