"""GPU: a patched mirror equals a fresh one (the mirror upkeep of the row edits, csrc/index.hip: live_mirrors / retile / mirrors_shrunk).

swap_remove, remove_rows and update_rows rewrite the touched 16-row tiles of every live Flat mirror instead of rebuilding it.  After each
edit the fp16 (tier 0) and split-bf16 (tier 1) keys of EVERY row must equal, bit for bit, those of an index built from scratch out of the
resulting rows and prepared the same way; the 8-bit mirror has no key dump whose bits a fresh build shares (its centre is sampled), so for
it the forced 8-bit search must return the fresh index's ids and distances with the mirror still valid, i.e. patched and not dropped.

Shape: 20 011 rows x 128 (the smallest the forced tiers take; 20 011 = 16 * 1250 + 11 = 192 * 104 + 43, ragged against both).  Row 5
carries the largest norm by far, survives every edit and is never updated, and new vectors are scaled by 0.5: both indexes then have one
xsq_max and with it one fp16 scale (asserted).  dx_abs / dx_rel are not compared: a fresh build measures them over fewer rows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 20011, 128
BIG = 5  # the row with the largest norm


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    return vdb


@pytest.fixture(scope="module")
def base():
    b = np.random.default_rng(61).standard_normal((N, DIM)).astype(np.float32)
    b[BIG] *= 4
    b.setflags(write=False)
    return b


def _swap_replay(n, seq):
    """original row ids, in table order, after swap_remove(i) for every i of `seq` in turn"""
    cur = np.arange(n)
    for i in seq:
        cur[i] = cur[-1]
        cur = cur[:-1]
    return cur


def _remove_replay(n, rows):
    """... after swap_remove on `rows` in descending order (what remove_rows leaves)"""
    return _swap_replay(n, sorted((int(r) for r in rows), reverse=True))


# four swap_removes in turn, n = 20011 -> 20007: inside the ragged last tile (20003, last = 20010); i == last (20009 of 20010 rows);
# tile 0 (3, last = 20008); the last row's tile but not the last row (20001, last = 20007)
SWAPS = (20003, 20009, 3, 20001)
# a block of 2001 rows across n' = 18010 (= 16 * 1125 + 10 = 192 * 93 + 154)
BLOCK = np.arange(17010, 19011)


def _update():
    rng = np.random.default_rng(62)
    inner = rng.permutation(np.arange(16, 20000))[:36]
    rows = np.concatenate([[1, 14, 20000, N - 1], inner])  # first and last tile, never row BIG
    return rows[rng.permutation(40)], (0.5 * rng.standard_normal((40, DIM))).astype(np.float32)


def _edits(base):
    """name -> (the edit, the table it leaves, positions in that table whose tiles were rewritten)"""
    rows, new = _update()
    after_u = base.copy()
    after_u[rows] = new

    def swaps(ix):
        for i in SWAPS:
            ix.swap_remove(i)

    return {
        "swap_remove": (swaps, base[_swap_replay(N, SWAPS)], [20003, 3, 20001, 20006, 0]),
        "remove_rows": (lambda ix: ix.remove_rows(BLOCK), base[_remove_replay(N, BLOCK)], [17010, 17500, 18009, 0, 18000]),
        "update_rows": (lambda ix: ix.update_rows(rows, new), after_u, [1, 14, 20000, N - 1, int(rows[7])]),
    }


def _prepared(vdb, rows):
    ix = vdb.GpuIndex(DIM, "l2sqr")
    ix.batch_add(rows)
    ix.set_param("flat_i8", 1)
    ix.prepare(all_tiers=True)
    assert ix.get_stat("flat_half_valid") == 1 and ix.get_stat("flat_bf16_mirror") == 1
    return ix


def _assert_keys_equal(patched, fresh, qs, tiers):
    for tier in tiers:
        kp, kf = patched.flat_shortlist_keys(qs, tier), fresh.flat_shortlist_keys(qs, tier)
        assert kp[3]["xsq_max"] == kf[3]["xsq_max"], tier  # one fp16 scale
        assert kp[0].shape == kf[0].shape == (len(qs), len(fresh))
        assert np.array_equal(kp[0].view(np.uint32), kf[0].view(np.uint32)), tier


@pytest.mark.parametrize("edit", ["swap_remove", "remove_rows", "update_rows"])
def test_fp16_and_bf16_keys_equal_a_fresh_build(vdb, base, edit):
    apply, after, touched = _edits(base)[edit]
    assert np.argmax((after.astype(np.float64) ** 2).sum(1)) == BIG  # the largest norm survived in place
    patched = _prepared(vdb, base)
    apply(patched)
    assert len(patched) == len(after)
    assert patched.get_stat("flat_half_valid") == 1 and patched.get_stat("flat_bf16_mirror") == 1  # kept in step, not dropped
    fresh = _prepared(vdb, after)
    qs = np.concatenate([after[touched], base[[77, 9000, 16000]]])
    _assert_keys_equal(patched, fresh, qs, (0, 1))
    patched.close()
    fresh.close()


def _forced_i8(vdb, rows, qs):
    ix = vdb.GpuIndex(DIM, "l2sqr")
    ix.batch_add(rows)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    ix.flat_knn(qs, 7)  # the 8-bit mirror is built and in step with the table
    assert ix.get_stat("flat_i8_valid") == 1
    return ix


@pytest.mark.parametrize("edit", ["swap_remove", "remove_rows", "update_rows"])
def test_i8_mirror_is_patched_and_answers_as_a_fresh_one(vdb, base, edit):
    apply, after, touched = _edits(base)[edit]
    rng = np.random.default_rng(63)
    at = np.concatenate([touched, rng.integers(0, len(after), 35)])  # queries at rewritten tiles: a stale tile would be visible
    qs = (after[at] + 1e-3 * rng.standard_normal((40, DIM))).astype(np.float32)
    patched = _forced_i8(vdb, base, qs)
    apply(patched)
    assert patched.get_stat("flat_i8_valid") == 1  # patched, not dropped for a rebuild
    before = patched.get_stat("flat_i8_queries")
    got = patched.flat_knn(qs, 7)
    assert patched.get_stat("flat_i8_queries") == before + 40
    fresh = _forced_i8(vdb, after, qs)
    want = fresh.flat_knn(qs, 7)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2].tolist() == want[2].tolist()
    patched.close()
    fresh.close()


def test_u8_index_bf16_keys_equal_a_fresh_build(vdb):
    """30-byte u8 rows re-tile through widened chunks: swap_remove, then remove_rows of a block across n' = 18009"""
    rng = np.random.default_rng(64)
    rows = rng.integers(0, 255, size=(N, 30), dtype=np.uint8)
    rows[BIG] = 255
    block = np.arange(17009, 19010)
    after = rows[_swap_replay(N, [20003])]
    after = after[_remove_replay(N - 1, block)]
    qs = np.concatenate([after[[20, 17009, 18008, 0]], rows[[20003, 19500]]]).astype(np.float32)
    patched = vdb.GpuIndex(30, "l2sqr", scalar="u8")
    patched.batch_add_u8(rows)
    patched.flat_shortlist_keys(qs, 1)  # builds the split-bf16 mirror
    assert patched.get_stat("flat_bf16_mirror") == 1
    patched.swap_remove(20003)
    patched.remove_rows(block)
    assert len(patched) == len(after) == 18009 and patched.get_stat("flat_bf16_mirror") == 1
    assert np.array_equal(patched.get_rows_u8(np.arange(len(after))), after)
    fresh = vdb.GpuIndex(30, "l2sqr", scalar="u8")
    fresh.batch_add_u8(after)
    _assert_keys_equal(patched, fresh, qs, (1,))
    patched.close()
    fresh.close()
