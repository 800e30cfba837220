"""CPU: the host model of the row edits (tests/edit_model.py) against the definitions it restates.

remove_rows == the literal swap_remove loop in descending order, and its net moves == vdb_remove_plan's (dst, src); labels travel with
their rows; rows added after a shrink are unlabelled, also where labelled rows stood before; the mask stamps follow the documented rule;
the step generator is a function of its seed and never draws an illegal step; the aimed queries find their rows.  Wall time: 6 s."""
import numpy as np
import pytest

import edit_model as em


def _table(n, dim=8, seed=1, u8=False, kind=em.L2SQR):
    m = em.EditModel(dim, kind, u8=u8, seed=seed)
    m.add(m.vectors(n, 0))
    return m


def _loop(model, ids):
    """the definition: swap_remove on `ids` in descending order, one call each"""
    for i in sorted((int(r) for r in ids), reverse=True):
        model.swap_remove(i)


def _id_sets(rng, n):
    n1 = lambda m: n - m  # noqa: E731
    m = int(rng.integers(0, n + 1))
    a = int(rng.integers(0, n + 1))
    return {
        "random": rng.permutation(n)[:m],
        "empty": np.zeros(0, dtype=np.int64),
        "all": np.arange(n),
        "last_tile": np.arange((n - 1) // 16 * 16 if n else 0, n),
        "tail": np.arange(n1(m // 2), n),  # entirely inside the old tail [n', n)
        "below": rng.permutation(n - min(m, n // 2))[:min(m, n // 2)],  # entirely below n'
        "block": np.arange(a, a + int(rng.integers(0, n - a + 1))),
    }


def test_remove_rows_is_the_swap_remove_loop_and_the_plan():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(1806)
    seen = {}
    for it in range(400):
        n = int(rng.integers(1, 301))
        for kind, ids in _id_sets(rng, n).items():
            a, b = _table(n, seed=it), _table(n, seed=it)
            for m in (a, b):
                m.set_labels(0, np.arange(n) % 7)
                m.set_labels_rows(np.arange(0, n, 3), [3], (np.arange(0, n, 3) + 100).astype(np.uint32))
            before = a.rows.copy()
            touch, (dst, src) = a.remove_rows(rng.permutation(ids))  # (any order)
            _loop(b, ids)
            assert np.array_equal(a.rows, b.rows) and len(a) == n - len(ids), (kind, n)
            assert all(np.array_equal(a.labels[c], b.labels[c]) for c in (0, 3)), (kind, n)
            pd, ps = vdb.remove_plan(n, np.sort(ids))
            assert np.array_equal(dst, pd) and np.array_equal(src, ps), (kind, n, ids)
            replay = before.copy()
            replay[pd.astype(np.int64)] = before[ps.astype(np.int64)]
            assert np.array_equal(replay[:len(a)], a.rows), (kind, n)
            assert sorted(touch.moved_to.tolist()) == sorted(pd.tolist())
            assert a.write_gen == (2 if len(ids) else 1)  # one call, one step; the empty list changes nothing
            seen[kind] = seen.get(kind, 0) + 1
    assert set(seen) == {"random", "empty", "all", "last_tile", "tail", "below", "block"} and min(seen.values()) == 400


def test_labels_follow_their_rows():
    n = 203
    m = _table(n)
    tag = np.arange(n, dtype=np.uint32) + 1000  # a label that names the row it was given to
    m.set_labels(0, tag)
    m.set_labels(3, tag[50:150] + 5000, first_row=50)
    stamp = m.rows.copy()
    m.remove_rows(np.arange(120, 190))  # across n' = 133
    m.swap_remove(0)
    m.swap_remove(len(m) - 1)
    for p in range(len(m)):
        origin = int(m.labels[0][p]) - 1000
        assert np.array_equal(m.rows[p], stamp[origin])
        assert m.labels[3][p] == (origin + 6000 if 50 <= origin < 150 else em.NONE)
    assert len(m) == n - 72 and len(set(m.labels[0].tolist())) == len(m)


def test_rows_added_after_a_shrink_are_unlabelled():
    m = _table(100)
    m.set_labels(0, np.full(100, 4, dtype=np.uint32))
    m.remove_rows(np.arange(40, 90))  # 50 rows left: positions 50 .. 99 held labelled rows
    m.add(m.vectors(80, 9))
    assert len(m) == 130 and (m.labels[0][:50] == 4).all() and (m.labels[0][50:] == em.NONE).all()
    assert m.label_counts(0, [4, em.NONE]).tolist() == [50, 80]
    assert 3 not in m.labels and (m.column(3) == em.NONE).all() and 3 not in m.labels  # reading brings no column to life
    m.set_labels_rows([129, 2], [3, 0], [[1, 2], [3, em.NONE]])
    assert m.labels[3][129] == 1 and m.labels[3][2] == 2 and m.labels[0][129] == 3 and m.labels[0][2] == em.NONE
    assert m.where([(3, 1), (0, 3)]).nonzero()[0].tolist() == [129]


def test_mask_stamps_follow_the_documented_rule():
    m = _table(100)
    s = m.mask_stamp()
    m.update_rows([3, 99], m.vectors(2, 5))
    m.set_labels(0, np.zeros(100, dtype=np.uint32))
    m.set_labels_rows([1], [3], [2])
    m.remove_rows([])
    assert m.mask_usable(s) and m.rowc_gen == 1  # vectors and labels changed, the set of rows did not
    for write in (lambda: m.add(m.vectors(1, 6)), lambda: m.swap_remove(5), lambda: m.remove_rows([7, 8])):
        s = m.mask_stamp()
        write()
        assert not m.mask_usable(s)
    s = m.mask_stamp()
    m.swap_remove(0)
    m.add(m.vectors(1, 7))  # the same row count again: still another set of rows
    assert not m.mask_usable(s)


def _legal(model, step, min_rows):
    op = model.expand(step)
    n = len(model)
    for ids in [a for a in op[1:2] if op[0] in ("remove_rows", "update_rows", "set_labels_rows")]:
        assert len(ids) and len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < n, step
    if op[0] == "swap_remove":
        assert 0 <= op[1] < n, step
    if op[0] == "set_labels":
        assert 0 <= op[3] and op[3] + len(op[2]) <= n and len(op[2]), step
    if op[0] in ("update_rows",):
        assert op[2].shape == (len(op[1]), model.dim)
    model.apply(op)
    assert len(model) >= min_rows, step


@pytest.mark.parametrize("u8", [False, True])
def test_generator_is_deterministic_and_legal(u8):
    kinds = set()
    for seed in range(40):
        n0 = (64, 70, 300, 5000)[seed % 4]
        runs = []
        for _ in range(2):
            m = _table(n0, seed=seed, u8=u8)
            steps = em.draw_steps(np.random.default_rng(seed), m, 14, min_rows=64)
            assert len(m) == n0 and m.log == []  # drawing changes nothing
            for st in steps:
                assert all(isinstance(x, (int, str, tuple)) and not isinstance(x, bool) for x in st), st  # plain, printable
                _legal(m, st, 64)
                kinds.add(st[0] + (":" + st[1] if st[0] == "remove_rows" else ""))
            runs.append((steps, m.rows.copy(), {c: v.copy() for c, v in m.labels.items()}))
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
        assert all(np.array_equal(runs[0][2][c], runs[1][2][c]) for c in runs[0][2])
        assert em.draw_steps(np.random.default_rng(seed + 1000), _table(n0, seed=seed, u8=u8), 14) != runs[0][0]
    want = {"add", "swap_remove", "remove_rows:block", "remove_rows:share", "remove_rows:last_tile", "set_labels", "set_labels_rows"}
    assert kinds == want | (set() if u8 else {"update_rows"})


@pytest.mark.parametrize("u8,kind", [(False, em.L2SQR), (False, em.COSINE), (True, em.L2SQR)])
def test_aimed_queries_find_their_rows(u8, kind):
    """... and the expectations are the oracle's: the filtered list is the full list cut to the allowed rows, the range holds its ball"""
    m = _table(1003, dim=32, seed=3, u8=u8, kind=kind)
    rng = np.random.default_rng(4)
    touch = m.remove_rows(np.arange(900, 960))[0]
    t2 = m.add(m.vectors(100, 11))
    touch.new_at = t2.new_at
    if not u8:
        t3 = m.update_rows([5, 940, 1000], m.vectors(3, 12))
        touch.new_at, touch.old_vecs = np.concatenate([touch.new_at, t3.new_at]), np.concatenate([touch.old_vecs, t3.old_vecs])
    qs, hit = m.queries(rng, touch, 48)
    assert qs.shape == (48, 32) and qs.dtype == m.rows.dtype and (hit >= 0).sum() >= 20 and (hit < 0).sum() >= 10
    assert set(range(1040, 1043)) <= set(hit.tolist()) and set(range(0, 16, 3)) <= set(hit.tolist())  # the last tile's rows, tile 0's
    oi, od, oc = m.knn(qs, 1003 + 40)
    assert (oc == len(m)).all()
    allow = np.arange(len(m)) % 3 != 1
    fi, fd, fc = m.knn(qs, em.K, allow)
    radius, lims, ri, rd = m.range(qs, em.K)
    for q in range(48):
        keep = allow[oi[q].astype(np.int64)]
        assert np.array_equal(fi[q], oi[q][keep][:em.K]) and np.array_equal(fd[q].view(np.uint32), od[q][keep][:em.K].view(np.uint32))
        ball = od[q] <= radius[q]
        assert np.array_equal(ri[int(lims[q]):int(lims[q + 1])], oi[q][ball]) and ball.sum() >= em.K


def test_a_broken_generator_does_not_pass_silently():
    """queries that are NOT at the rows they claim to aim at (here: shifted by one) trip the model's own assertion"""
    class Broken(em.EditModel):
        def _near(self, rng, vecs):
            return np.roll(super()._near(rng, vecs), 1, axis=0)

    m = Broken(16, seed=5)
    m.add(m.vectors(200, 0))
    with pytest.raises(AssertionError, match="misses"):
        m.queries(np.random.default_rng(6), m.add(m.vectors(20, 1)), 48)
