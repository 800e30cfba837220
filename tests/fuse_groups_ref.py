"""The rule of the document-level fused search (include/vdbhip.h, vdb_flat_knn_fused_groups / vdb_fuse_groups_device) as a loop over
np.float32 scalars: one rounding per operation, no FMA, every fold in ascending list order.  tests/test_fuse_groups_ref_cpu.py verifies it
on hand-computed cases and against a brute-force restatement; the GPU tests compare the kernel with it bit for bit.

A list is (ids, dists): the entries that count, in rank order (the caller cuts at min(count, ld)).  `group_of(id)` names the group of a
row by any hashable value; label_groups() builds it from a label column the way the library reads one: the code, or -- for a row without
one -- the row itself, in a key space of its own."""
import numpy as np

from fuse_ref import F, bits, order_key  # noqa: F401  (bits: for the users of this module)

RRF, MIN, SUM = "rrf", "min", "sum"
LABEL_NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000


def label_groups(labels, id_offset=0):
    """group_of for a label column (None: never written): ("l", code), or ("r", row) for an unlabelled row"""
    def group_of(i):
        row = int(i) - int(id_offset)
        code = LABEL_NONE if labels is None else int(labels[row])
        return ("r", row) if code == LABEL_NONE else ("l", code)
    return group_of


def first_occurrences(ids, dists, group_of):
    """group -> (rank among the groups of the list, row id, distance) at the group's first position"""
    seen = {}
    for i, d in zip(ids, dists):
        g = group_of(i)
        if g not in seen:
            seen[g] = (len(seen), int(i), F(d))
    return seen


def fuse_groups(lists, group_of, k, mode=RRF, weights=None, c=60.0, trunc_len=None):
    """-> (representative ids, scores as np.float32, exact): the first min(k, groups) entries of the fused answer.  trunc_len None: no
    list is a truncated one."""
    c = F(c)
    occ = [first_occurrences(ids, dists, group_of) if len(ids) else None for ids, dists in lists]
    last = [F(dists[len(ids) - 1]) if len(ids) else None for ids, dists in lists]
    groups = list(dict.fromkeys(g for o in occ for g in (o or {})))
    score, rep = {}, {}
    with np.errstate(all="ignore"):
        for g in groups:
            acc, best = F(0.0), None  # best: (order key, s, row, distance)
            for s, o in enumerate(occ):
                if o is None:
                    continue  # a list with no counted entry is skipped in every fold
                if g in o:
                    rank, row, d = o[g]
                    if best is None or order_key(d) < best[0]:
                        best = (order_key(d), s, row, d)
                    if mode == RRF:
                        w = F(1.0) if weights is None else F(weights[s])
                        den = F(F(rank + 1) + c)
                        term = F(w / den)
                        acc = F(acc + term)
                    elif mode == SUM:
                        acc = F(acc + d)
                elif mode == SUM:
                    acc = F(acc + last[s])
            rep[g] = best[2]
            if mode == MIN:
                acc = best[3]
            elif mode == SUM and np.isnan(acc):
                acc = np.array(NAN_BITS, dtype=np.uint32).view(np.float32)[()]
            score[g] = acc
        if mode == RRF:
            ranked = sorted(groups, key=lambda g: (order_key(-score[g]), rep[g]))
        else:
            ranked = sorted(groups, key=lambda g: (order_key(score[g]), rep[g]))
    n_all = len(ranked)
    ranked = ranked[:k]
    trunc = [last[s] for s, (ids, _) in enumerate(lists) if trunc_len is not None and len(ids) and len(ids) >= trunc_len]
    exact = not trunc and k > 0  # (k == 0: nothing is fetched or ranked, and `exact` is 0)
    if trunc and mode == MIN and k > 0 and min(k, n_all) == k:
        kth = order_key(score[ranked[k - 1]])
        exact = all(kth < order_key(f) for f in trunc)
    return (np.array([rep[g] for g in ranked], dtype=np.uint64), np.array([score[g] for g in ranked], dtype=np.float32), int(exact))
