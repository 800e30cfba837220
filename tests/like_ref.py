"""The reference of the search by example rows (vdb_like_queries, vdb_flat_knn_like, vdb_drop_listed_device) for the tests: a Python loop
over list entries with np.float32 scalars -- one rounding per operation, as the contract in include/vdbhip.h states it.  It uses
nothing of the library under test.  tests/test_like_ref_cpu.py checks it on hand-computed cases, so the GPU tests compare against a
reference that is itself verified.

Per element j of a query: sp = +0.0, then sp = sp + row[j] for each positive in list order (a strict left fold; a repeat counts as often
as it appears); ap = sp / |P|.  With negatives an is the same fold and divide over them and query[j] = (ap + ap) - an; without,
query[j] = ap."""
import numpy as np


def _mean(rows, ids, j):
    s = np.float32(0.0)
    for r in ids:
        s = np.float32(s + rows[int(r), j])
    return np.float32(s / np.float32(len(ids)))


def like_query(rows, pos, neg=()):
    """the query vector (float32 [dim]) of the example rows `pos` / `neg` (row numbers into `rows`, in list order)"""
    rows = np.asarray(rows, dtype=np.float32)
    pos, neg = list(pos), list(neg)
    assert len(pos) >= 1
    out = np.zeros(rows.shape[1], dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(rows.shape[1]):
            ap = _mean(rows, pos, j)
            if neg:
                an = _mean(rows, neg, j)
                twice = np.float32(ap + ap)
                out[j] = np.float32(twice - an)
            else:
                out[j] = ap
    return out


def like_queries(rows, positives, negatives=None):
    """like_query per query -> float32 [nq][dim]"""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.zeros((len(positives), rows.shape[1]), dtype=np.float32)
    for q, pos in enumerate(positives):
        out[q] = like_query(rows, pos, negatives[q] if negatives is not None else ())
    return out


def drop_listed(ids, listed, k):
    """the positions kept by the drop walk: the list `ids` is walked as given, an entry is kept unless its id is listed, the walk stops
    at k kept"""
    listed = [int(x) for x in listed]
    kept = []
    for p, i in enumerate(ids):
        if len(kept) >= int(k):
            break
        if int(i) not in listed:
            kept.append(p)
    return kept


def same_floats(a, b):
    """bit-for-bit equality of two float32 arrays, except that a NaN matches any NaN: IEEE 754 leaves the sign and payload of a NaN an
    operation produces to the implementation (x86 makes inf - inf the negative quiet NaN, the GPU the positive one)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
