"""A host model of one Flat table under row edits, for the sequence tests (tests/test_edit_sequences_gpu.py, tools/fuzz_mutate.py).

Plain numpy: the model holds the rows in table order, the label columns and the two generation counters that decide whether a RowMask
is still usable, and it restates the library's write semantics:

  add(rows)                      rows appended, unlabelled (LABEL_NONE) in every live column
  swap_remove(i)                 row i takes the last row's vector and labels, the table loses its last row (VecSet::swap_remove)
  remove_rows(ids)               swap_remove on `ids` in DESCENDING order (MetadataVecTable::delete)
  update_rows(ids, vecs)         new vectors in place; labels, row ids and masks stay
  set_labels / set_labels_rows   a column comes to life with LABEL_NONE everywhere on its first write

Mask rule (include/vdbhip.h): a mask is a set of rows.  add / swap_remove / remove_rows change the set (write_gen moves: masks made before
are refused), update_rows and the label writes do not (the masks stay; update_rows moves rowc_gen: their row-constant copies are stale).

Expected answers come from the CPU oracle on the model's CURRENT rows (oracle.flat_knn_batch; a u8 table through its exactly widened
rows, which is what dist_u8 folds), so nothing the library computes enters an expectation.

Steps are small printable tuples (sizes, positions and seeds, never arrays): `expand` turns one into a concrete op against the model's
state, `apply` runs the op on the model, `apply_to_index` runs the same op on a GpuIndex.  The list of steps is the bug report: every
check's assert message carries `model.log`.
"""
import numpy as np

NONE = 0xFFFFFFFF  # LABEL_NONE (labels.py) / VDB_LABEL_NONE (k_labels.hip): the row carries no value in that column
L2SQR, COSINE = 0, 1
NOISE = 1e-3
K = 7
COLUMNS = (0, 3)  # the label columns the generator writes
CODES = 5         # ... with codes 0 .. 4 (and LABEL_NONE)


class Touch:
    """what one op changed: positions that now hold NEW vectors, the OLD vectors it overwrote or removed, positions rows were MOVED to"""

    def __init__(self, new_at=(), old_vecs=None, moved_to=()):
        self.new_at = np.asarray(new_at, dtype=np.int64).reshape(-1)
        self.old_vecs = old_vecs
        self.moved_to = np.asarray(moved_to, dtype=np.int64).reshape(-1)


class EditModel:
    def __init__(self, dim, kind=L2SQR, u8=False, scale=1.0, offset=None, seed=0):
        self.dim, self.kind, self.u8, self.scale = int(dim), int(kind), bool(u8), float(scale)
        self.offset = np.zeros(dim) if offset is None else np.asarray(offset, dtype=np.float64)
        self.rows = np.zeros((0, dim), dtype=np.uint8 if u8 else np.float32)
        self.labels = {}
        self.write_gen = 0  # moves when the SET of rows changes: masks made before are refused
        self.rowc_gen = 0   # moves when vectors change in place: masks stay, their row constants are rebuilt
        self.seed = int(seed)
        self.log = []

    def __len__(self):
        return len(self.rows)

    # ---- data ------------------------------------------------------------------------------------------------------------------------
    def vectors(self, m, seed):
        """m fresh rows of this table's distribution, a function of (model seed, seed) alone"""
        rng = np.random.default_rng([self.seed, int(seed)])
        if self.u8:
            return rng.integers(0, 256, size=(m, self.dim), dtype=np.uint8)
        return ((rng.standard_normal((m, self.dim)) + self.offset) * self.scale).astype(np.float32)

    def wide(self, rows=None):
        """f32 rows as the distances see them (u8 elements widen exactly)"""
        r = self.rows if rows is None else rows
        return np.ascontiguousarray(r, dtype=np.float32)

    # ---- writes ----------------------------------------------------------------------------------------------------------------------
    def add(self, rows):
        rows = np.asarray(rows, dtype=self.rows.dtype).reshape(-1, self.dim)
        n = len(self)
        if len(rows) == 0:
            return Touch()
        self.rows = np.concatenate([self.rows, rows])
        for c in self.labels:
            self.labels[c] = np.concatenate([self.labels[c], np.full(len(rows), NONE, dtype=np.uint32)])
        self.write_gen += 1
        return Touch(new_at=np.arange(n, n + len(rows)))

    def swap_remove(self, i):
        i, last = int(i), len(self) - 1
        assert 0 <= i <= last
        old = self.rows[i:i + 1].copy()
        self.rows[i] = self.rows[last]
        self.rows = self.rows[:last].copy()
        for c in self.labels:
            self.labels[c][i] = self.labels[c][last]
            self.labels[c] = self.labels[c][:last].copy()
        self.write_gen += 1
        return Touch(old_vecs=old, moved_to=[i] if i < last else [])

    def remove_rows(self, ids):
        """the descending swap_remove loop; returns the Touch and the net moves (dst, src) a caller of remove_rows gets"""
        ids = sorted((int(r) for r in np.asarray(ids).reshape(-1)), reverse=True)
        assert len(set(ids)) == len(ids) and (not ids or ids[0] < len(self))
        if not ids:
            return Touch(), (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
        old = self.rows[ids[::-1]].copy()
        origin = np.arange(len(self))  # origin[p]: where the row now at p stood before the call; the loop runs on these, the rows follow once
        for i in ids:
            origin[i] = origin[-1]
            origin = origin[:-1]
        self.rows = self.rows[origin]
        for c in self.labels:
            self.labels[c] = self.labels[c][origin]
        self.write_gen += 1  # one call, one step
        moved = np.flatnonzero(origin != np.arange(len(origin)))
        order = moved[::-1]  # dst descending, as vdb_remove_plan lists them
        return Touch(old_vecs=old, moved_to=moved), (order.astype(np.uint64), origin[order].astype(np.uint64))

    def update_rows(self, ids, vecs):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        assert not self.u8, "update_rows needs f32 rows"
        assert len(np.unique(ids)) == len(ids) and (len(ids) == 0 or (ids.min() >= 0 and ids.max() < len(self)))
        if len(ids) == 0:
            return Touch()
        old = self.rows[ids].copy()
        self.rows[ids] = np.asarray(vecs, dtype=np.float32).reshape(len(ids), self.dim)
        self.rowc_gen += 1
        return Touch(new_at=ids, old_vecs=old)

    def _column(self, c):
        if c not in self.labels:
            self.labels[c] = np.full(len(self), NONE, dtype=np.uint32)
        return self.labels[c]

    def column(self, c):
        """the codes of column c without bringing it to life"""
        return self.labels[c] if c in self.labels else np.full(len(self), NONE, dtype=np.uint32)

    def set_labels(self, column, codes, first_row=0):
        codes = np.asarray(codes, dtype=np.uint32).reshape(-1)
        assert first_row + len(codes) <= len(self)
        self._column(int(column))[first_row:first_row + len(codes)] = codes
        return Touch()

    def set_labels_rows(self, ids, columns, codes):
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        codes = np.asarray(codes, dtype=np.uint32).reshape(len(columns), len(ids))
        assert len(np.unique(ids)) == len(ids) and len(set(columns)) == len(columns)
        for j, c in enumerate(columns):
            self._column(int(c))[ids] = codes[j]
        return Touch()

    # ---- masks -----------------------------------------------------------------------------------------------------------------------
    def mask_stamp(self):
        """what a mask made now remembers"""
        return (self.write_gen, len(self))

    def mask_usable(self, stamp):
        return stamp == (self.write_gen, len(self))

    def where(self, terms):
        """bool over the rows: label column c == code for EVERY (c, code)"""
        allow = np.ones(len(self), dtype=np.bool_)
        for c, code in terms:
            allow &= self.column(int(c)) == np.uint32(code)
        return allow

    # ---- expected answers ------------------------------------------------------------------------------------------------------------
    def knn(self, qs, k, allow=None, nthreads=8):
        """(idx u64 [nq][k], dist f32 [nq][k], cnt [nq]) of the oracle; under `allow` (bool over the rows): on the allowed rows, ids mapped back"""
        from oracle import oracle as O

        qs = self.wide(qs)
        if allow is None:
            return O.flat_knn_batch(self.wide(), qs, k, self.kind, nthreads=nthreads)
        ids = np.flatnonzero(allow)
        oi, od, oc = O.flat_knn_batch(self.wide(self.rows[ids]), qs, k, self.kind, nthreads=nthreads)
        back = np.zeros_like(oi)
        for q in range(len(qs)):
            c = int(oc[q])
            back[q, :c] = ids[oi[q, :c].astype(np.int64)]
        return back, od, oc

    def range(self, qs, k, allow=None, extra=5):
        """(radius, lims, ids, dists): each query's radius is the oracle's k-th distance, its ball the oracle rows at or below it; the
        oracle's list of k + extra rows is asserted to hold the whole ball, so no tolerance enters (test_update_rows_gpu._expect_range)"""
        oi, od, oc = self.knn(qs, k + extra, allow)
        assert (oc == k + extra).all(), "the table holds fewer rows than the range check needs"
        radius = od[:, k - 1].copy()
        lims, ids, ds = [0], [], []
        for q in range(len(oi)):
            cut = int((od[q] <= radius[q]).sum())
            assert k <= cut < od.shape[1], ("the oracle's list does not hold the whole ball", q, self.log)
            ids.append(oi[q, :cut])
            ds.append(od[q, :cut])
            lims.append(lims[-1] + cut)
        return radius, np.array(lims, dtype=np.uint64), np.concatenate(ids).astype(np.uint64), np.concatenate(ds)

    def label_counts(self, column, codes, allow=None):
        col = self.column(int(column))
        col = col if allow is None else col[allow]
        return np.array([int((col == np.uint32(c)).sum()) for c in codes], dtype=np.uint64)

    # ---- queries aimed at what an op touched -------------------------------------------------------------------------------------------
    def _near(self, rng, vecs):
        if self.u8:  # one element off by one: still nearest to its row
            v = np.array(vecs, dtype=np.int16)
            col = rng.integers(0, self.dim, len(v))
            v[np.arange(len(v)), col] += np.where(v[np.arange(len(v)), col] < 128, 1, -1)
            return v.astype(np.uint8)
        return (np.asarray(vecs, dtype=np.float32) + NOISE * rng.standard_normal((len(vecs), self.dim))).astype(np.float32)

    def queries(self, rng, touch, nq=48):
        """nq queries: at the NEW vectors `touch` left, at the OLD vectors it overwrote or removed, at rows moved into holes, at the rows
        of the ragged last tile and of tile 0 (each + 1e-3 noise), and random ones.  For the queries at rows of the table the oracle's
        nearest row must be that row (or an exact copy of it): asserted here, so that a broken generator cannot pass silently."""
        n = len(self)

        def some(a, m):
            a = np.asarray(a)
            return a if len(a) <= m else a[np.unique(np.linspace(0, len(a) - 1, m).astype(np.int64))]

        last0 = (n - 1) // 16 * 16
        at = np.concatenate([some(touch.new_at, 10), some(touch.moved_to, 8), some(np.arange(last0, n), 6), some(np.arange(0, min(16, n)), 6)]).astype(np.int64)
        at = at[at < n]
        parts, hit = [self._near(rng, self.rows[at])], at.tolist()
        if touch.old_vecs is not None and len(touch.old_vecs):
            old = some(np.arange(len(touch.old_vecs)), 10)
            parts.append(self._near(rng, touch.old_vecs[old]))
            hit += [-1] * len(old)
        m = max(nq - len(hit), 3)
        parts.append(self.vectors(m, int(rng.integers(1 << 30))))  # random: as far from every row as the rows are from each other
        hit += [-1] * m
        qs, hit = np.concatenate(parts)[:nq], np.array(hit[:nq], dtype=np.int64)
        aimed = np.flatnonzero(hit >= 0)
        if len(aimed):
            oi, _, _ = self.knn(qs[aimed], 1)
            for j, q in enumerate(aimed):
                got = int(oi[j, 0])
                assert got == hit[q] or np.array_equal(self.rows[got], self.rows[hit[q]]), ("a query aimed at a row misses it", int(hit[q]), got, self.log)
        return qs, hit

    # ---- steps -----------------------------------------------------------------------------------------------------------------------
    def expand(self, step):
        """a step tuple -> the concrete op (name, arrays ...) against the CURRENT state"""
        name, n = step[0], len(self)
        if name == "add":  # ("add", m, seed, dup): m fresh rows; dup >= 0: the first of them is an exact copy of row dup
            _, m, seed, dup = step
            vecs = self.vectors(m, seed)
            if dup >= 0:
                vecs[0] = self.rows[dup]
            return ("add", vecs)
        if name == "swap_remove":
            return ("swap_remove", int(step[1]))
        if name == "remove_rows":  # ("remove_rows", "block", first, m) / ("share", m, seed) / ("last_tile",)
            kind = step[1]
            if kind == "block":
                ids = np.arange(step[2], step[2] + step[3])
            elif kind == "share":
                ids = np.random.default_rng(step[3]).permutation(n)[:step[2]]
            else:
                ids = np.arange((n - 1) // 16 * 16, n)
            return ("remove_rows", ids.astype(np.int64))
        if name == "update_rows":  # ("update_rows", m, seed): m random rows + row 1 + the last row, shuffled
            _, m, seed = step
            rng = np.random.default_rng(seed)
            ids = rng.permutation(np.unique(np.concatenate([rng.permutation(n)[:m], [min(1, n - 1), n - 1]])))
            return ("update_rows", ids.astype(np.int64), self.vectors(len(ids), seed))
        if name == "set_labels":  # ("set_labels", column, first_row, count, seed)
            _, col, first, count, seed = step
            return ("set_labels", col, _codes(seed, count), first)
        if name == "set_labels_rows":  # ("set_labels_rows", m, columns, seed)
            _, m, cols, seed = step
            ids = np.random.default_rng(seed).permutation(n)[:m]
            return ("set_labels_rows", ids.astype(np.int64), tuple(cols), _codes(seed + 1, m * len(cols)).reshape(len(cols), m))
        raise ValueError(step)

    def apply(self, op, note=None):
        """runs a concrete op on the model -> its Touch; the op is logged (in its short form) for the assert messages"""
        self.log.append(note if note is not None else describe(op))
        name = op[0]
        if name == "remove_rows":
            return self.remove_rows(op[1])[0]
        return getattr(self, name)(*op[1:])


def _codes(seed, m):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, CODES, m).astype(np.uint32)
    c[rng.random(m) < 0.1] = NONE
    return c


def describe(op):
    """an op in one short line: arrays as their length and ends"""
    def short(a):
        if isinstance(a, np.ndarray):
            flat = a.reshape(-1)
            return f"<{a.shape} {flat[0]}..{flat[-1]}>" if a.ndim == 1 and len(flat) else f"<{a.shape}>"
        return repr(a)
    return f"{op[0]}(" + ", ".join(short(a) for a in op[1:]) + ")"


def apply_to_index(ix, op):
    """the same op on a GpuIndex (or anything with its methods)"""
    name = op[0]
    if name == "add":
        return ix.batch_add_u8(op[1]) if op[1].dtype == np.uint8 else ix.batch_add(op[1])
    if name == "set_labels":
        return ix.set_labels(op[1], op[2], op[3])
    return getattr(ix, name)(*op[1:])


def draw_steps(rng, model, n_steps, min_rows=64, labels=True):
    """n_steps write steps as plain tuples, legal for a table that starts with len(model) rows and has every earlier step applied: ids
    distinct and below the row count at that step, never fewer than `min_rows` rows left (the checks ask for K + 5 of them, also under a
    mask).  Only the row count is simulated: `model` is not changed."""
    n = len(model)
    assert n >= min_rows
    kinds = ["add", "add", "swap_remove", "remove_block", "remove_share", "remove_last_tile", "update_rows"]
    if model.u8:
        kinds.remove("update_rows")
    if labels:
        kinds += ["set_labels", "set_labels_rows"]
    steps = []
    while len(steps) < n_steps:
        kind = kinds[int(rng.integers(len(kinds)))]
        seed = int(rng.integers(1 << 30))
        room = n - min_rows  # rows that may go
        if kind == "add":
            m = int(rng.choice([1, 3, 200, 2500]))
            steps.append(("add", m, seed, int(rng.integers(n)) if rng.random() < 0.3 else -1))
            n += m
        elif kind == "swap_remove" and room >= 1:
            steps.append(("swap_remove", int(rng.choice([n - 1, (n - 1) // 16 * 16, rng.integers(n), rng.integers(min(16, n))]))))
            n -= 1
        elif kind == "remove_block" and room >= 1:
            m = int(min(room, rng.choice([1, 17, 500, max(n // 10, 1)])))
            first = int(rng.integers(0, n - m + 1)) if rng.random() < 0.5 else max(n - m - int(rng.integers(0, m + 1)), 0)  # (or: across the new end)
            steps.append(("remove_rows", "block", first, m))
            n -= m
        elif kind == "remove_share" and room >= 1:
            m = int(min(room, max(int(n * rng.choice([0.01, 0.3, 0.6])), 1)))
            steps.append(("remove_rows", "share", m, seed))
            n -= m
        elif kind == "remove_last_tile" and room >= n - (n - 1) // 16 * 16:
            steps.append(("remove_rows", "last_tile"))
            n = (n - 1) // 16 * 16
        elif kind == "update_rows":
            steps.append(("update_rows", int(min(n, rng.choice([1, 40, max(n // 10, 1)]))), seed))
        elif kind == "set_labels":
            count = int(rng.integers(1, n + 1))
            steps.append(("set_labels", int(rng.choice(COLUMNS)), int(rng.integers(0, n - count + 1)), count, seed))
        elif kind == "set_labels_rows":
            steps.append(("set_labels_rows", int(rng.integers(1, min(n, 300) + 1)), COLUMNS if rng.random() < 0.5 else COLUMNS[:1], seed))
    return steps


# ---- checks of an index against the model: bit for bit, the step list in every message -----------------------------------------------------
def _same_knn(got, exp, model, what):
    (gi, gd, gc), (ei, ed, ec) = got, exp
    assert np.array_equal(np.asarray(gc, dtype=np.uint64), ec), (what, "counts", model.log)
    bad = np.flatnonzero((gi != ei.astype(np.uint64)).any(1) | (gd.view(np.uint32) != ed.view(np.uint32)).any(1))
    assert len(bad) == 0, (what, "queries", bad.tolist(), "got", gi[bad[0]].tolist(), "want", ei[bad[0]].tolist(), model.log)


def check_knn(ix, model, qs, k=K, what="knn"):
    got = ix.flat_knn_u8(qs, k) if model.u8 else ix.flat_knn(qs, k)
    _same_knn(got, model.knn(qs, k), model, what)


def check_filtered(ix, model, qs, mask, allow, k=K, what="filtered knn"):
    _same_knn(ix.flat_knn_filtered(qs, k, mask), model.knn(qs, k, allow), model, what)


def check_range(ix, model, qs, k=K, mask=None, allow=None, what="range"):
    radius, el, ei, ed = model.range(qs, k, allow)
    gl, gi, gd = ix.range_search(qs, radius) if mask is None else ix.range_search(qs, radius, mask=mask)
    assert np.array_equal(gl, el), (what, "lims", model.log)
    assert np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), (what, model.log)


def check_rows(ix, model, ids, what="rows"):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    assert len(ix) == len(model), (what, "len", len(ix), len(model), model.log)
    if len(ids) == 0:
        return
    got = ix.get_rows_u8(ids) if model.u8 else ix.get_rows(ids).view(np.uint32)
    want = model.rows[ids] if model.u8 else model.rows[ids].view(np.uint32)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (what, "rows differ at", ids[bad][:8].tolist(), model.log)


def check_labels(ix, model, what="labels"):
    for c, col in model.labels.items():
        got = ix.get_labels(c)
        bad = np.flatnonzero(got != col)
        assert len(got) == len(col) and len(bad) == 0, (what, "column", c, "rows", bad[:8].tolist(), model.log)
        codes = list(range(CODES)) + [NONE]
        assert np.array_equal(ix.label_counts(c, codes), model.label_counts(c, codes)), (what, "counts of column", c, model.log)
