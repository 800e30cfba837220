"""CPU: tests/rescore_ref.py on seven rows whose answers are written out by hand (none is produced by the reference).

labels   row 0, 1: code 5 | row 2, 3, 5: code 9 | row 4: none | row 6: code 7
s0       4.0  1.0  2.0  2.0  0.5  NaN  NaN
s1       1.0  3.0  2.0  0.25 8.0  6.0  6.0

question A  (s0, s1) over the candidates 1, 0, 3, 4, 1, 6: row 0 and the second 1 are duplicates of group 5.  Group 5: s0 -> row 1 (1.0),
            s1 -> row 0 (1.0): the keys tie across the sub-queries and the first s wins -- representative 1.  Group 9: s0 -> rows 2 and
            3 tie at 2.0 and the lower row wins, the NaN of row 5 is last; s1 -> row 3 (0.25).  Group 7: NaN + 6.0.
question B  (s0) over 3, 6 (a third id is past the count): group 9 scores 2.0 and row 2 represents it, not the candidate 3.
question C  (s0 under a mask that hides rows 0 and 1, s1 unmasked) over 0, 4: group 5 folds +inf + 1.0 under SUM and is 1.0 under MIN.
question D  (s0, s1 under a mask that hides rows 0, 1 and 4) over 1, 4, 3: two groups without an allowed row: +inf under SUM and MIN,
            represented by their candidates, ordered by them behind the one real score."""
import numpy as np
import pytest

import rescore_ref as R
from fuse_ref import order_key

NONE = R.LABEL_NONE
LAB = np.array([5, 5, 9, 9, NONE, 9, 7], dtype=np.uint32)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
S0 = np.array([4.0, 1.0, 2.0, 2.0, 0.5, NAN, NAN], dtype=np.float32)
S1 = np.array([1.0, 3.0, 2.0, 0.25, 8.0, 6.0, 6.0], dtype=np.float32)
DM = np.stack([S0, S1, S0, S0, S1, S0, S1])
LIMS = np.array([0, 2, 3, 5, 7], dtype=np.uint64)
CANDS = np.array([[1, 0, 3, 4, 1, 6], [3, 6, 2, 0, 0, 0], [0, 4, 0, 0, 0, 0], [1, 4, 3, 0, 0, 0]], dtype=np.uint64)
COUNTS = np.array([6, 2, 2, 3], dtype=np.uint64)
EVERY = np.ones(7, dtype=np.bool_)
ALLOWS = [EVERY, np.array([0, 0, 1, 1, 1, 1, 1], dtype=np.bool_), np.array([0, 0, 1, 1, 0, 1, 1], dtype=np.bool_)]
MASK_OF = np.array([0, 0, 0, 1, 0, 2, 2], dtype=np.uint32)
ROWS = 7 + 4 + 3 + 6  # A: 2 + 3 + 1 + 1 | B: 3 + 1 | C: 2 + 1 | D: 2 + 1 + 3

# per mode and question: [(representative, score)], written out by hand
HAND = {
    "sum": [[(1, 2.0), (3, 2.25), (4, 8.5), (6, NAN)], [(2, 2.0), (6, NAN)], [(4, 8.5), (0, INF)], [(3, 2.25), (1, INF), (4, INF)]],
    "min": [[(3, 0.25), (4, 0.5), (1, 1.0), (6, 6.0)], [(2, 2.0), (6, NAN)], [(4, 0.5), (0, 1.0)], [(3, 0.25), (1, INF), (4, INF)]],
}


def _bits(x):
    b = int(np.array(x, dtype=np.float32).view(np.uint32))
    return R.NAN_BITS if np.isnan(x) else b


@pytest.mark.parametrize("mode", ["sum", "min"])
@pytest.mark.parametrize("k", [6, 3, 1])  # 6: above the number of groups of every question
@pytest.mark.parametrize("off", [0, (1 << 33) + 3])
def test_hand_computed_call(mode, k, off):
    idx, bits, cnt, rows = R.expect(DM, LAB, LIMS, CANDS + np.uint64(off), COUNTS, k, mode, allows=ALLOWS, mask_of=MASK_OF, id_offset=off)
    assert idx.shape == (4, k) and bits.shape == (4, k) and idx.dtype == np.uint64 and bits.dtype == np.uint32 and rows == ROWS
    for q, hand in enumerate(HAND[mode]):
        take = min(k, len(hand))
        assert cnt[q] == take
        assert idx[q].tolist() == [r + off for r, _ in hand[:take]] + [0] * (k - take), (q, idx[q])
        assert bits[q].tolist() == [_bits(s) for _, s in hand[:take]] + [0] * (k - take), (q, bits[q].view(np.float32))


def test_unmasked_questions_and_a_column_never_written():
    idx, bits, cnt, rows = R.expect(DM[:3], LAB, LIMS[:3], CANDS[:2], COUNTS[:2], 4, "sum")
    assert cnt.tolist() == [4, 2] and rows == 11 and idx.tolist() == [[1, 3, 4, 6], [2, 6, 0, 0]]
    # every candidate row a group of its own: question A is rows 1, 0, 3, 4, 6 (the second 1 is the same row twice)
    idx, bits, cnt, rows = R.expect(DM[:3], None, LIMS[:3], CANDS[:2], COUNTS[:2], 6, "sum")
    assert cnt.tolist() == [5, 2] and rows == 7
    assert idx[0, :5].tolist() == [3, 1, 0, 4, 6] and bits[0, :5].tolist() == [_bits(x) for x in (2.25, 4.0, 5.0, 8.5, NAN)]
    assert idx[1, :2].tolist() == [3, 6] and bits[1, :2].tolist() == [_bits(2.0), R.NAN_BITS]


def test_no_candidates_and_k_zero():
    idx, bits, cnt, rows = R.expect(DM[:3], LAB, LIMS[:3], CANDS[:2], np.zeros(2, np.uint64), 2, "min")
    assert cnt.tolist() == [0, 0] and rows == 0 and not idx.any() and not bits.any()
    idx, bits, cnt, rows = R.expect(DM[:3], LAB, LIMS[:3], CANDS[:2], COUNTS[:2], 0, "sum")
    assert idx.shape == (2, 0) and cnt.tolist() == [0, 0] and rows == 0


def test_order_keys_is_order_key():
    """negative distances (cosine can give one) order before both zeros, which are equal; every NaN is one key, the last"""
    vals = np.array([-1.0, -1e-7, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf, np.nan, -np.nan], dtype=np.float32)
    keys = R.order_keys(vals)
    assert keys.dtype == np.uint32 and keys.tolist() == [order_key(v) for v in vals]
    assert keys.tolist() == sorted(keys.tolist()) and keys[2] == keys[3] and keys[8] == keys[9] and len(set(keys.tolist())) == 8
