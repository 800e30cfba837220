"""The rule of the exact late-interaction rescoring of candidate documents (include/vdbhip.h, vdb_flat_rescore_groups /
vdb_flat_rescore_groups_device) over a dense f32 distance table dm[sub-query][row] (the GPU tests take it from oracle.flat_knn_batch at
k = n, so the pair distances are the CPU oracle's and only the grouping, the minima, the fold and the order are restated here).
tests/test_rescore_ref_cpu.py pins it on hand-computed cases; the GPU tests compare the kernels with it bit for bit.

  - the candidates of a question dedupe to groups: the rows that share the candidate's label code, or -- for a row without one -- the
    row itself; the same group twice counts once, at its first occurrence;
  - per sub-query the group's smallest (order_key(distance), row) over the rows that sub-query's mask allows;
  - "sum": a strict np.float32 left fold of those distances in ascending sub-query order, +inf where no row is allowed; "min": the
    smallest of them (+inf when no sub-query has an allowed row);
  - the representative: the row of the smallest (key, s, row), or the first-occurring candidate when no row is allowed at all;
  - the groups leave ordered by (order_key(score), representative); every NaN score is the one NaN 0x7FC00000.

The minima are found with numpy over a group's rows (argmin returns the first of equal keys, and the members are ascending rows); the
fold and the order are loops over np.float32 scalars: one rounding per operation."""
import numpy as np

from fuse_ref import F, order_key

SUM, MIN = "sum", "min"
LABEL_NONE = 0xFFFFFFFF
NAN_BITS = 0x7FC00000
INF = F(np.inf)


def order_keys(d):
    """fuse_ref.order_key over an array: uint32 keys of f32 distances (-0 == +0, every NaN equal and last)"""
    with np.errstate(all="ignore"):
        u = (np.asarray(d, dtype=np.float32) + F(0.0)).view(np.uint32)
    u = np.where((u & 0x7FFFFFFF) > 0x7F800000, np.uint32(NAN_BITS), u)
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


class Groups:
    """the groups of a label column (None: never written -- every row is a group of its own), members in ascending row order"""

    def __init__(self, labels, n=None):
        self.labels = None if labels is None else np.asarray(labels, dtype=np.uint32)
        self.n = len(self.labels) if n is None else n
        self._rows = {}
        if self.labels is not None:
            order = np.argsort(self.labels, kind="stable")
            codes, start = np.unique(self.labels[order], return_index=True)
            for c, a, b in zip(codes.tolist(), start.tolist(), start.tolist()[1:] + [len(order)]):
                if c != LABEL_NONE:
                    self._rows[c] = order[a:b]

    def of(self, row):
        """(group name, its rows)"""
        code = LABEL_NONE if self.labels is None else int(self.labels[row])
        return (("r", row), np.array([row], dtype=np.int64)) if code == LABEL_NONE else (("l", code), self._rows[code])


def question(dq, groups, cand_rows, k, mode, allow=None):
    """ONE question: dq [S][n] its sub-queries' distances to every row, cand_rows its counted candidates (LOCAL rows, in list order),
    allow None or S boolean row masks (None entries: every row) -> (representatives, scores as np.float32, candidate rows evaluated): the
    first min(k, groups) of the answer"""
    S = len(dq)
    keys = order_keys(dq)
    seen, out, rows = set(), [], 0
    for r in (int(x) for x in cand_rows):
        name, members = groups.of(r)
        if name in seen:
            continue
        seen.add(name)
        rows += len(members)
        acc, best = F(0.0), None  # best: (order key, s, row, distance)
        for s in range(S):
            ms = members if allow is None or allow[s] is None else members[np.asarray(allow[s])[members]]
            if len(ms) == 0:
                with np.errstate(all="ignore"):
                    acc = F(acc + INF)
                continue
            at = int(np.argmin(keys[s][ms]))  # (the first of equal keys: the lowest row)
            row, d = int(ms[at]), F(dq[s][ms[at]])
            with np.errstate(all="ignore"):
                acc = F(acc + d)
            if best is None or (int(keys[s][row]), s, row) < best[:3]:
                best = (int(keys[s][row]), s, row, d)
        rep = r if best is None else best[2]
        score = acc if mode == SUM else (INF if best is None else best[3])
        if np.isnan(score):
            score = np.array(NAN_BITS, dtype=np.uint32).view(np.float32)[()]
        out.append((order_key(score), rep, score))
    out.sort(key=lambda t: t[:2])
    out = out[:k]
    return np.array([t[1] for t in out], dtype=np.uint64), np.array([t[2] for t in out], dtype=np.float32), rows


def expect(dm, labels, lims, cands, counts, k, mode, allows=None, mask_of=None, id_offset=0):
    """A whole call as the library lays it out: dm [lims[-1]][n]; cands [nq][ld] the ids as passed (id_offset included), of which the
    first counts[q] count; allows a list of boolean row masks and mask_of [lims[-1]] the mask of each sub-query (both None: no masks)
    -> (idx [nq][k] u64, score bits [nq][k] u32, count [nq] u64, candidate rows evaluated); slots past a count are zero"""
    nq = len(lims) - 1
    groups = labels if isinstance(labels, Groups) else Groups(labels, n=dm.shape[1])
    idx, bits, cnt, rows = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.uint32), np.zeros(nq, np.uint64), 0
    for q in range(nq):
        a, b = int(lims[q]), int(lims[q + 1])
        allow = None if allows is None else [allows[int(mask_of[j])] for j in range(a, b)]
        local = (np.asarray(cands[q][:int(counts[q])]).astype(np.uint64) - np.uint64(id_offset)).astype(np.int64)
        ids, scores, r = question(dm[a:b], groups, local, k, mode, allow)
        rows += r if k else 0  # (k == 0: nothing is ranked and no pair is evaluated)
        cnt[q] = len(ids)
        idx[q, :len(ids)] = ids + np.uint64(id_offset)
        bits[q, :len(ids)] = scores.view(np.uint32)
    return idx, bits, cnt, rows
