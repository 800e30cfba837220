"""Plain references and constructed inputs for the k-NN shard merges (test helper: test_merge_topk_cpu.py, test_merge_topk_gpu.py,
test_pq_merge_gpu.py).

The references are written from the contract, not from the library's host merges: the CPU tests compare the two.

Order image of a distance (csrc/common.hpp, "total order of CandidatePair"): -0 is +0, every NaN is the one canonical +NaN, which
orders after +inf, negatives order below positives; unsigned integer order of the image is the order of the distances.  A merged
pair comes back with the distance its image decodes to, so -0.0 returns as +0.0 and any NaN as 0x7FC00000.
A pair key is image << 32 | id (id < 2^32); PAIR_NONE = 2^64 - 1 pads a key row."""
import bisect

import numpy as np

PAIR_NONE = 0xFFFFFFFFFFFFFFFF
ID_TOP = (1 << 32) - 1

# the tie values of the Flat inputs, as bit patterns (NaN payloads survive): +0, -0, the smallest subnormal, -1.5, 0.25, 1,
# the float after 1, FLT_MAX, +inf, the canonical NaN, a negative NaN with a payload
VALUE_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0xBFC00000, 0x3E800000, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000,
                       0x7FC00000, 0xFFC00123], dtype=np.uint32)
NAN_BITS = (0x7FC00000, 0xFFC00123)
NEG_INF_BITS = 0xFF800000

# (S, k): the one-launch kernel (k <= 64) -- S*k = 63, 64, 65, more than 64 shards, more than one round of 64 pairs
SHAPES_K64 = [(1, 1), (2, 1), (3, 10), (1, 64), (2, 32), (7, 9), (5, 13), (64, 64), (65, 63), (300, 7)]
# the scratch-list branch: every list width R in {2, 4, 8, 16} at both ends of its range of k, more than one list
SHAPES_LISTS = [(2, 65), (3, 100), (8, 128), (3, 129), (5, 256), (2, 257), (4, 512), (3, 513), (9, 1000), (2, 1024)]
SHAPE_LARGEST = (64, 1024)  # at nq = 2
NQS = (1, 5, 33)

# (S, efk, k) of the PQ merge: k <= 64, the wave lists beyond, the heap replay + row sort beyond 1024
PQ_SHAPES = [(1, 1, 1), (2, 10, 10), (4, 100, 10), (8, 64, 64), (3, 65, 65), (33, 200, 64), (2, 1000, 1000), (3, 1024, 1024),
             (2, 1025, 1025), (4, 3000, 1500), (2, 3000, 10)]
PQ_NQS = (1, 7)


def order_image(d):
    """u32 image of f32 distances whose unsigned order is the distance order"""
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, 0x7FC00000, u)  # every NaN -> the canonical +NaN
    u = np.where(u == 0x80000000, 0, u)  # -0 -> +0
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def image_to_f32(o):
    o = np.asarray(o, dtype=np.uint64)
    u = np.where(o & 0x80000000, o & 0x7FFFFFFF, ~o & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


def merge_topk_ref(dists, ids, counts, k):
    """dists [S][nq][k] f32, ids [S][nq][k] u64, counts [S][nq] u64 -> (idx [nq][k] u64, dist [nq][k] f32, cnt [nq] u64): per query
    the first min(count, k) pairs of every shard, sorted by (image, id), the first k of them; pads are id 0 / distance +0.0"""
    S, nq = counts.shape
    oi = np.zeros((nq, k), dtype=np.uint64)
    od = np.zeros((nq, k), dtype=np.float32)
    oc = np.zeros(nq, dtype=np.uint64)
    img = order_image(dists)
    for q in range(nq):
        take = [slice(0, min(int(counts[s, q]), k)) for s in range(S)]
        im = np.concatenate([img[s, q, take[s]] for s in range(S)])
        idq = np.concatenate([ids[s, q, take[s]] for s in range(S)])
        order = np.lexsort((idq, im))[:k]
        c = len(order)
        oi[q, :c] = idq[order]
        od[q, :c] = image_to_f32(im[order])
        oc[q] = c
    return oi, od, oc


def pq_merge_resort_ref(adc, exact, k):
    """adc / exact [S][nq][efk] u64 pair keys -> (idx [nq][k] u64, dist [nq][k] f32, cnt [nq] u64): per query the pairs whose ADC key
    is not PAIR_NONE, sorted by ADC key, the first efk of them; ResultSet::add with capacity k replayed over their exact keys in that
    order (insert while not full; when full the worst leaves only for a strictly smaller DISTANCE word); ascending"""
    S, nq, efk = adc.shape
    oi = np.zeros((nq, k), dtype=np.uint64)
    od = np.zeros((nq, k), dtype=np.float32)
    oc = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        a = adc[:, q, :].reshape(-1)
        e = exact[:, q, :].reshape(-1)
        valid = a != np.uint64(PAIR_NONE)
        a, e = a[valid], e[valid]
        e = e[np.argsort(a, kind="stable")][:efk]
        kept = []  # ascending keys
        for key in e.tolist():
            if len(kept) >= k:
                if (key >> 32) >= (kept[-1] >> 32):
                    continue
                kept.pop()
            bisect.insort(kept, key)
        c = len(kept)
        keys = np.array(kept, dtype=np.uint64)
        oi[q, :c] = keys & np.uint64(0xFFFFFFFF)
        od[q, :c] = image_to_f32(keys >> np.uint64(32))
        oc[q] = c
    return oi, od, oc


def same(got, exp, what=""):
    """bit-exact: ids, distance bit patterns, counts"""
    gi, gd, gc = (np.asarray(x) for x in got)
    ei, ed, ec = exp
    assert np.array_equal(gc.astype(np.uint64), ec), (what, "counts", gc, ec)
    assert np.array_equal(gi.view(np.uint64) if gi.dtype == np.int64 else gi, ei), (what, "ids")
    assert gd.dtype == np.float32 and np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), (what, "distance bits")


def _unique_ids(rng, t, id_base):
    """t distinct ids, half of them low, half just below 2^32 with 2^32 - 1 among them (t >= 1), in random order"""
    n_hi = t - t // 2
    lo = rng.choice(4 * t, size=t // 2, replace=False).astype(np.uint64)
    hi = np.concatenate([[0], 1 + rng.choice(4 * t, size=n_hi - 1, replace=False)]).astype(np.uint64)
    out = np.concatenate([lo, np.uint64(ID_TOP) - hi])
    rng.shuffle(out)
    return out + np.uint64(id_base)


def flat_case(S, nq, k, seed, id_base=0):
    """Constructed per-shard lists for the Flat merge: (dists [S][nq][k] f32, ids [S][nq][k] u64, counts [S][nq] u64).

    Per shard and query ascending by (distance, id), as the contract says.  Distances from VALUE_BITS (ties are the rule); ids unique
    per query, reaching 2^32 - 1 (+ id_base), dealt so that shard order is not id order; where a query has pairs, one of them is
    (NaN, 2^32 - 1).  Counts from {0, 1, k - 1, k}; every slot past the count is poison: distance -inf and an id no list uses.
    Query q is of kind q % 5:
      0  counts drawn per shard; the pairs dealt in DESCENDING shard order (the highest shard holds the smallest (distance, id) pairs)
      1  every shard full, some reporting a count above k; the pairs dealt to the shards at random (interleaved)
      2  fewer than k pairs in total (counts 0 and 1), interleaved
      3  every shard 0
      4  counts drawn per shard, some above k, interleaved"""
    rng = np.random.default_rng(seed)
    d_bits = np.full((S, nq, k), NEG_INF_BITS, dtype=np.uint32)
    ids = np.zeros((S, nq, k), dtype=np.uint64)
    counts = np.zeros((S, nq), dtype=np.uint64)
    poison = (1 << 31) + id_base  # (the lists' ids lie within 4 * S * k of 0 and of 2^32)
    ids[:] = (np.uint64(poison) + np.arange(S * nq * k, dtype=np.uint64)).reshape(S, nq, k)
    for q in range(nq):
        kind = q % 5
        if kind in (0, 4):
            c = rng.choice(np.array([0, 1, k - 1, k]), size=S)
        elif kind == 1:
            c = np.full(S, k)
        elif kind == 2:
            c = np.zeros(S, dtype=np.int64)
            c[rng.permutation(S)[:min(S, k - 1)]] = 1
        else:
            c = np.zeros(S, dtype=np.int64)
        t = int(c.sum())
        reported = c.astype(np.uint64)
        if kind in (1, 4):  # a count above k is read as k
            over = (c == k) & (rng.random(S) < 0.5)
            reported = np.where(over, np.where(rng.random(S) < 0.5, k + 1, (1 << 40) + 7), c).astype(np.uint64)
        counts[:, q] = reported
        if t == 0:
            continue
        pid = _unique_ids(rng, t, id_base)
        pbits = VALUE_BITS[rng.integers(len(VALUE_BITS), size=t)]
        pbits[pid == np.uint64(ID_TOP + id_base)] = NAN_BITS[q % 2]
        order = np.lexsort((pid, order_image(pbits.view(np.float32))))
        pid, pbits = pid[order], pbits[order]
        owner = np.repeat(np.arange(S), c)  # owner[i]: the shard that receives the i-th pair of the query's global order
        if kind == 0:
            owner = owner[::-1]
        else:
            rng.shuffle(owner)
        for s in range(S):
            mine = owner == s
            ids[s, q, :int(c[s])] = pid[mine]
            d_bits[s, q, :int(c[s])] = pbits[mine]
    return d_bits.view(np.float32), ids, counts


def pack_blocks(ex, dists, ids, counts):
    """the S per-rank blocks of an all-gather buffer in ShardExchange's layout (offsets taken from `ex`), as one uint8 array
    pre-filled with 0xFF: whatever the layout leaves between the distances and the counts is poison"""
    S = dists.shape[0]
    buf = np.full((S, ex.block), 0xFF, dtype=np.uint8)
    n = ex.nq * ex.k
    for s in range(S):
        buf[s, ex.off_ids:ex.off_ids + n * 8] = ids[s].reshape(-1).view(np.uint8)
        buf[s, ex.off_dists:ex.off_dists + n * 4] = dists[s].reshape(-1).view(np.uint8)
        buf[s, ex.off_counts:ex.off_counts + ex.nq * 8] = counts[s].view(np.uint8)
    return buf.reshape(-1)


# ADC distances of the PQ inputs (few values: ties across shards, the id decides) and the four exact distances
PQ_ADC_VALUES = np.array([-0.5, 0.0, -0.0, 0.125, 0.5, 1.0, 3.0, np.inf], dtype=np.float32)
PQ_EXACT_VALUES = np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32)


def pq_case(S, nq, efk, k, seed):
    """Constructed key rows for the PQ merge: (adc [S][nq][efk] u64, exact [S][nq][efk] u64).

    ADC rows ascending, ids unique per query (up to 2^32 - 1) and interleaved over the shards, ADC distances from PQ_ADC_VALUES,
    PAIR_NONE tails (both rows) of different lengths; the exact key at a position carries the same id and one of four distances.
    Query q is of kind q % 3: 0 = row lengths drawn from {0, 1, efk / 2, efk - 1, efk}; 1 = every row full except one shard that is
    entirely PAIR_NONE (S > 1); 2 = fewer than k valid entries in total."""
    rng = np.random.default_rng(seed)
    adc = np.full((S, nq, efk), PAIR_NONE, dtype=np.uint64)
    exact = np.full((S, nq, efk), PAIR_NONE, dtype=np.uint64)
    for q in range(nq):
        kind = q % 3
        if kind == 0:
            c = rng.choice(np.array([0, 1, efk // 2, efk - 1, efk]), size=S)
        elif kind == 1:
            c = np.full(S, efk)
            if S > 1:
                c[rng.integers(S)] = 0
        else:
            c = np.zeros(S, dtype=np.int64)
            left = k - 1
            for s in rng.permutation(S):
                c[s] = min(efk, int(rng.integers(0, left + 1)))
                left -= int(c[s])
        t = int(c.sum())
        if t == 0:
            continue
        pid = _unique_ids(rng, t, 0)
        a = (order_image(PQ_ADC_VALUES[rng.integers(len(PQ_ADC_VALUES), size=t)]) << np.uint64(32)) | pid
        e = (order_image(PQ_EXACT_VALUES[rng.integers(len(PQ_EXACT_VALUES), size=t)]) << np.uint64(32)) | pid
        order = np.argsort(a, kind="stable")
        a, e = a[order], e[order]
        owner = np.repeat(np.arange(S), c)
        rng.shuffle(owner)
        for s in range(S):
            mine = owner == s
            adc[s, q, :int(c[s])] = a[mine]
            exact[s, q, :int(c[s])] = e[mine]
    return adc, exact
