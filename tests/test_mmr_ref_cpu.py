"""CPU: tests/mmr_ref.py -- the reference walk of the diversified k-NN (maximal marginal relevance) that the GPU tests compare against
-- checked without a GPU against a brute-force restatement: the explicit F x F matrix of oracle.dist pair distances, and per step the
min over ALL selected positions recomputed from that matrix and an argmin under (score, position).  A few hundred random cases with
NaN and inf components, duplicate rows and zero rows, both metrics, lambda in {0, 0.25, 0.5, 1}; the lambda = 1 => prefix property; the
symmetry of the pair distance bit for bit, which the kernel relies on."""
import numpy as np
import pytest

import mmr_ref as R

KINDS = (0, 1)  # oracle.L2SQR, oracle.COSINE
LAMBDAS = (0.0, 0.25, 0.5, 1.0)


def _brute(d, M, k, lam):
    """the restatement: nothing incremental -- every step recomputes m[p] over all selected s, in selection order"""
    F = len(d)
    kk = min(k, F)
    if kk == 0:
        return []
    lam = np.float32(lam)
    mu = np.float32(np.float32(1.0) - lam)
    sel = [0]
    while len(sel) < kk:
        cand = []
        for p in range(F):
            if p in sel:
                continue
            m = R.INF
            for s in sel:
                if M[p, s] < m:
                    m = M[p, s]
            cand.append((R.score(lam, mu, d[p], m), p))
        best = cand[0]
        for c in cand[1:]:
            if c[0] < best[0] or (c[0] == best[0] and c[1] < best[1]):
                best = c
        sel.append(best[1])
    return sel


def _rows(rng, n, dim, special):
    rows = (rng.standard_normal((n, dim)) * rng.choice([0.01, 1.0, 100.0])).astype(np.float32)
    if special:
        for _ in range(int(rng.integers(0, 4))):  # duplicates: D = 0, score ties decided by position
            a, b = rng.integers(0, n, 2)
            rows[a] = rows[b]
        if rng.random() < 0.5:
            rows[rng.integers(0, n)] = 0.0  # a zero row: Cosine's clamped denominator
        for v in (np.nan, np.inf, -np.inf):
            if rng.random() < 0.4:
                rows[rng.integers(0, n), rng.integers(0, dim)] = v
    return rows


def _cases():
    rng = np.random.default_rng(4101)
    out = []
    for i in range(240):
        n = int(rng.integers(1, 24))
        dim = int(rng.choice([1, 3, 4, 7, 16]))
        rows = _rows(rng, n, dim, special=i % 2 == 1)
        q = rng.standard_normal(dim).astype(np.float32)
        out.append((rows, q, KINDS[i % 2 if i % 4 < 2 else 1 - i % 2], LAMBDAS[(i // 2) % 4], int(rng.integers(0, n + 2))))
    return out


def _order(rows, q, kind):
    """(row ids, distances) in the oracle's full order: ascending by (distance, id), NaN last"""
    from oracle import oracle as O

    oi, od = O.flat_knn(rows, q, len(rows), kind)
    assert len(oi) == len(rows)
    return oi.astype(np.int64), od


def test_incremental_walk_equals_brute_force():
    n_special = n_diverse = 0
    for rows, q, kind, lam, k in _cases():
        ids, d = _order(rows, q, kind)
        rd = R.RowDist(rows, kind)
        F = len(ids)
        M = np.array([[rd(ids[p], ids[s]) for s in range(F)] for p in range(F)], dtype=np.float32).reshape(F, F)
        got = R.walk_rows(rd, ids, d, k, lam)
        assert got == _brute(d, M, k, lam), (kind, lam, k)
        assert len(got) == min(k, F) and len(set(got)) == len(got) and (not got or got[0] == 0)
        n_special += bool(np.isnan(M).any() or np.isinf(M).any())
        n_diverse += got != list(range(len(got)))
    assert n_special >= 30 and n_diverse >= 30  # the cases reach NaN / inf pair distances, and orders other than the plain one


def test_smaller_k_is_a_prefix():
    """greedy: no step depends on k, so the selection at k is the first k entries of the selection of the whole list"""
    for rows, q, kind, lam, _ in _cases()[::6]:
        ids, d = _order(rows, q, kind)
        rd = R.RowDist(rows, kind)
        whole = R.walk_rows(rd, ids, d, len(ids), lam)
        for k in range(len(ids) + 1):
            assert R.walk_rows(rd, ids, d, k, lam) == whole[:k]


def test_lambda_one_is_the_prefix_of_the_plain_order():
    """on rows without NaN or inf: lambda = 1 selects positions 0, 1, .., k - 1 -- the plain search at the same k"""
    rng = np.random.default_rng(4102)
    for i in range(40):
        n, dim = int(rng.integers(1, 30)), int(rng.choice([2, 4, 9]))
        rows = _rows(rng, n, dim, special=False)
        if i % 3 == 0 and n > 2:
            rows[1] = rows[0]  # equal distances: the tie goes to the lower position, which is the plain order
        q = rng.standard_normal(dim).astype(np.float32)
        for kind in KINDS:
            ids, d = _order(rows, q, kind)
            k = int(rng.integers(1, n + 1))
            assert R.walk_rows(R.RowDist(rows, kind), ids, d, k, 1.0) == list(range(k))


def test_lambda_zero_is_farthest_first():
    rows = np.array([[0, 0], [0.1, 0], [5, 0], [5.1, 0], [0, 7]], dtype=np.float32)
    ids, d = _order(rows, np.zeros(2, dtype=np.float32), 0)
    assert ids.tolist() == [0, 1, 2, 3, 4]
    assert R.walk_rows(R.RowDist(rows, 0), ids, d, 3, 0.0) == [0, 4, 3]  # the farthest from {0}, then the farthest from {0, 4}
    assert R.walk_rows(R.RowDist(rows, 0), ids, d, 3, 1.0) == [0, 1, 2]
    # 0.25: score = 0.25 d - 0.75 m.  After {0}, m = d: -0.5 d, the farthest (4, then 3).  Then row 2 is a near-copy of the selected
    # row 3 (6.25 - 0.0075) and loses to row 1 (0.0025 - 0.0075)
    assert R.walk_rows(R.RowDist(rows, 0), ids, d, 5, 0.25) == [0, 4, 3, 1, 2]
    assert R.mmr_walk(np.array([0, 1, 1], np.float32), lambda p, s: np.float32(0), 3, 0.5) == [0, 1, 2]  # equal scores: position decides


@pytest.mark.parametrize("kind", KINDS)
def test_pair_distance_is_symmetric_bit_for_bit(kind):
    rng = np.random.default_rng(4103 + kind)
    for dim in (1, 3, 4, 20, 960):
        rows = _rows(rng, 12, dim, special=True)
        rd = R.RowDist(rows, kind)
        for a in range(12):
            for b in range(12):
                x, y = rd(a, b), rd(b, a)
                assert (np.isnan(x) and np.isnan(y)) or x.view(np.uint32) == y.view(np.uint32), (kind, dim, a, b)


def test_nan_scores_count_as_inf_and_ties_go_to_the_lowest_position():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # every pair distance NaN: m stays +inf, mu * inf = inf, score -inf for mu > 0 -- all equal, positions in order
    assert R.mmr_walk(np.array([1, 2, 3, 4], np.float32), lambda p, s: nan, 4, 0.5) == [0, 1, 2, 3]
    # lambda = 1: mu = 0, 0 * inf = NaN -> +inf for every position: positions in order
    assert R.mmr_walk(np.array([1, 5, 3, 4], np.float32), lambda p, s: nan, 4, 1.0) == [0, 1, 2, 3]
    # a NaN list distance: its score is NaN -> +inf, behind every finite score, before nothing
    assert R.mmr_walk(np.array([1, nan, 3, 2], np.float32), lambda p, s: np.float32(1), 4, 1.0) == [0, 3, 2, 1]
    # +inf == +inf: the lower position
    assert R.mmr_walk(np.array([1, inf, inf], np.float32), lambda p, s: np.float32(1), 3, 1.0) == [0, 1, 2]
    # -0 == +0
    assert R.mmr_walk(np.array([0, 0.0, -0.0], np.float32), lambda p, s: np.float32(0), 3, 1.0) == [0, 1, 2]
    assert R.mmr_walk(np.array([0, -0.0, 0.0], np.float32), lambda p, s: np.float32(0), 3, 1.0) == [0, 1, 2]
    assert R.mmr_walk(np.array([], np.float32), lambda p, s: nan, 3, 0.5) == [] and R.mmr_walk(np.array([1], np.float32), None, 0, 0.5) == []
