"""The reference of the diversified k-NN (maximal marginal relevance; vdb_flat_knn_mmr, vdb_mmr_select_device) for the tests: a Python
walk in np.float32 arithmetic -- one rounding per operation, as the contract in include/vdbhip.h states it -- over the CPU oracle's pair
distances (oracle.dist).  It uses nothing of the library under test.  tests/test_mmr_ref_cpu.py checks the incremental walk below
against a brute-force restatement (the explicit F x F matrix and an argmin per step), so the GPU tests compare against a reference that
is itself verified.

For one query: d[p] is the distance the search reports for list position p, D(p, s) the distance between the ROWS at positions p and s.
Position 0 is selected first; every later step gives each unselected p the score (lam * d[p]) - (mu * m[p]), mu = 1 - lam, m[p] = the
smallest D(p, s) over the selected s (m starts at +inf and takes D only if D < m: a NaN D is ignored; a NaN score counts as +inf), and
selects the smallest score, ties to the lowest position, until min(k, F) are selected."""
import numpy as np

INF = np.float32(np.inf)


class RowDist:
    """D(a, b) = oracle.dist(kind, rows[a], rows[b]) as np.float32, remembered per ordered pair (no symmetry is assumed here)"""

    def __init__(self, rows, kind):
        from oracle import oracle as O

        self._O, self.kind = O, kind
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self._memo = {}

    def __call__(self, a, b):
        key = (int(a), int(b))
        v = self._memo.get(key)
        if v is None:
            v = self._memo[key] = np.float32(self._O.dist(self.kind, self.rows[key[0]], self.rows[key[1]]))
        return v


def score(lam, mu, d, m):
    with np.errstate(all="ignore"):
        rel = np.float32(lam) * np.float32(d)
        div = np.float32(mu) * np.float32(m)
        s = np.float32(rel - div)
    return INF if np.isnan(s) else s


def mmr_walk(d, pair, k, lam):
    """positions selected from a list with distances d (f32 [F]); pair(p, s) = D between the rows at positions p and s.  Incremental:
    a step evaluates only D(p, position selected last) and folds it into m[p]."""
    d = np.asarray(d, dtype=np.float32)
    F = len(d)
    kk = min(int(k), F)
    if kk == 0:
        return []
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    m = np.full(F, INF, dtype=np.float32)
    taken = np.zeros(F, dtype=np.bool_)
    sel = [0]
    taken[0] = True
    while len(sel) < kk:
        last = sel[-1]
        best, best_s = -1, INF
        for p in range(F):
            if taken[p]:
                continue
            D = pair(p, last)
            if D < m[p]:
                m[p] = D
            s = score(lam, mu, d[p], m[p])
            if best < 0 or s < best_s:  # (strict: the first of equal scores stays)
                best, best_s = p, s
        sel.append(best)
        taken[best] = True
    return sel


def walk_rows(rd, rows, d, k, lam):
    """mmr_walk over a list of ROWS of rd (a RowDist)"""
    rows = [int(r) for r in rows]
    return mmr_walk(d, lambda p, s: rd(rows[p], rows[s]), k, lam)


def expect(rd, lists, dists, counts, k, lam, id_offset=0):
    """(idx, dist, cnt) [nq][max(k, 1)] of a call over lists of LOCAL rows: the selected pairs in selection order, zeros behind them"""
    nq, kk = len(lists), max(int(k), 1)
    idx = np.zeros((nq, kk), dtype=np.uint64)
    dist = np.zeros((nq, kk), dtype=np.float32)
    cnt = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        F = int(counts[q])
        rows = np.asarray(lists[q][:F], dtype=np.int64)
        dq = np.asarray(dists[q][:F], dtype=np.float32)
        sel = walk_rows(rd, rows, dq, k, lam)
        cnt[q] = len(sel)
        idx[q, :len(sel)] = rows[sel].astype(np.uint64) + np.uint64(id_offset)
        dist[q, :len(sel)] = dq[sel]
    return idx, dist, cnt
