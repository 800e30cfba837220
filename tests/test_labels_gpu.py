"""GPU: the label columns of an index (vdb_index_labels_set / _get, csrc/k_labels.hip: k_label_fill, k_label_move) stay in step with
the rows through add, swap_remove and remove_rows.  A numpy twin of two columns is kept beside the index and get_labels is compared
with it, exactly, after every step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
COLS = (0, 11)


class _Twin:
    def __init__(self, ix, dim, rng):
        self.ix, self.dim, self.rng = ix, dim, rng
        self.cols = {c: np.zeros(0, dtype=np.uint32) for c in COLS}

    def check(self, what):
        n = len(self.ix)
        for c in COLS:
            assert len(self.cols[c]) == n, what
            assert np.array_equal(self.ix.get_labels(c), self.cols[c]), (what, c)
        if n > 3:  # a sub-range
            assert np.array_equal(self.ix.get_labels(COLS[1], first_row=1, count=n - 3), self.cols[COLS[1]][1:n - 2]), what
        assert np.array_equal(self.ix.get_labels(5), np.full(n, NONE, dtype=np.uint32)), what  # never written

    def add(self, count, u8=False):
        if u8:
            self.ix.batch_add_u8(self.rng.integers(0, 256, size=(count, self.dim), dtype=np.uint8))
        else:
            self.ix.batch_add(self.rng.random((count, self.dim)).astype(np.float32))
        for c in COLS:  # the new rows carry no label
            self.cols[c] = np.concatenate([self.cols[c], np.full(count, NONE, dtype=np.uint32)])

    def set(self, c, first, count):
        codes = self.rng.integers(0, 7, size=count).astype(np.uint32)
        self.ix.set_labels(c, codes, first_row=first)
        self.cols[c][first:first + count] = codes

    def swap_remove(self, i):
        self.ix.swap_remove(i)
        for c in COLS:
            self.cols[c][i] = self.cols[c][-1]
            self.cols[c] = self.cols[c][:-1].copy()

    def remove(self, rows):
        dst, src = self.ix.remove_rows(rows)
        n1 = len(self.cols[COLS[0]]) - len(rows)
        for c in COLS:
            self.cols[c][dst.astype(np.int64)] = self.cols[c][src.astype(np.int64)]  # (src >= n1 > dst: no move reads another's target)
            self.cols[c] = self.cols[c][:n1].copy()
        return dst, src


def _walk(scalar, dim, n0, n1, n2):
    """n0 rows -> labels -> grow to n1 -> single removals -> scattered / contiguous bulk removals down to n2 -> everything -> add again"""
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(dim, "l2sqr", scalar=scalar)
    u8 = scalar == "u8"
    t = _Twin(ix, dim, np.random.default_rng(n0 + n1))
    try:
        assert ix.get_stat("label_columns") == 0
        t.add(n0, u8)
        t.check("fresh rows")
        assert ix.get_stat("label_columns") == 0  # reading allocates nothing
        base_bytes = ix.get_stat("hbm_bytes_per_row")
        t.set(COLS[0], 0, n0)
        assert ix.get_stat("label_columns") == 1 and ix.get_stat("hbm_bytes_per_row") == base_bytes + 4
        t.set(COLS[1], 3, n0 - 10)  # a column written only in part, after the rows existed: NONE elsewhere
        assert ix.get_stat("label_columns") == 2 and ix.get_stat("hbm_bytes_per_row") == base_bytes + 8
        t.check("set on a sub-range")
        gen_mask = ix.make_mask_where([(COLS[0], 1)])
        t.set(COLS[0], 5, 4)  # writing labels leaves the mask valid (it is a set of rows)
        assert len(gen_mask) >= 0 and gen_mask.rows()[1].size == len(gen_mask)
        gen_mask.close()
        t.check("rewritten range")
        t.add(n1 - n0, u8)
        t.check("batch_add: the new rows read NONE")
        t.set(COLS[1], n0 - 2, n1 - n0)
        t.check("labels across the old end")
        t.swap_remove(n1 // 2)
        t.check("swap_remove of a middle row")
        t.swap_remove(len(ix) - 1)
        t.check("swap_remove of the last row")
        n = len(ix)
        scattered = np.unique(t.rng.choice(n, size=(n - n2) // 2, replace=False))
        dst, src = t.remove(scattered)
        assert len(dst) > 0
        t.check("remove_rows of a scattered set")
        n = len(ix)
        block = np.arange(5, 5 + (n - n2))
        t.remove(block)
        assert len(ix) == n2
        t.check("remove_rows of a contiguous block")
        if not u8:  # filtered k-NN needs f32 rows: the masks of the surviving labels answer
            mk = ix.make_mask_where([(COLS[0], 2)])
            assert np.array_equal(mk.rows()[1], np.flatnonzero(t.cols[COLS[0]] == 2))
            mk.close()
        t.remove(np.arange(n2))
        assert len(ix) == 0
        t.check("remove_rows of everything")
        assert ix.get_stat("label_columns") == 2
        t.add(40, u8)
        t.check("add after emptying")
        t.set(COLS[0], 10, 20)
        t.check("labels after emptying")
    finally:
        ix.close()


@pytest.mark.parametrize("scalar", ("f32", "u8"))
def test_columns_follow_the_rows(scalar):
    _walk(scalar, 64, 600, 900, 120)  # dim 64: the MFMA mirrors' dimension, so the bulk removal runs beside their upkeep


@pytest.mark.parametrize("scalar", ("f32", "u8"))
def test_columns_across_tile_and_block_boundaries(scalar):
    _walk(scalar, 8, 250, 270, 17)  # 250 -> 270 crosses a 16-row tile and the 256-row block of the fill / move kernels; 17: one past a tile


def test_add_keeps_the_index_when_a_column_cannot_grow():
    """growth of the columns is reserved before add_rows changes anything: a failed allocation leaves rows and labels as they were.
    One-byte rows: 400 + 200 of them ask 1 KiB of the row buffer and nothing of the norms' (4 KiB since the first add), but the
    column's 2 KiB must double to 4 KiB -- the one allocation of the call past the 4000-byte limit set for it."""
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(1, "l2sqr", scalar="u8")
    try:
        rng = np.random.default_rng(2)
        rows = rng.integers(0, 256, size=(400, 1), dtype=np.uint8)
        ix.batch_add_u8(rows)
        lab = rng.integers(0, 4, size=400).astype(np.uint32)
        ix.set_labels(3, lab)
        ix.set_param("debug_alloc_fail_over", 4000)
        try:
            with pytest.raises(vdb.VdbError, match="out of memory"):
                ix.batch_add_u8(rng.integers(0, 256, size=(200, 1), dtype=np.uint8))
        finally:
            ix.set_param("debug_alloc_fail_over", 0)
        assert len(ix) == 400 and np.array_equal(ix.get_labels(3), lab)
        assert all(int(ix.row_u8(i)[0]) == int(rows[i, 0]) for i in (0, 199, 399))
        ix.batch_add_u8(rng.integers(0, 256, size=(200, 1), dtype=np.uint8))
        assert len(ix) == 600 and np.array_equal(ix.get_labels(3), np.concatenate([lab, np.full(200, NONE, dtype=np.uint32)]))
    finally:
        ix.close()
