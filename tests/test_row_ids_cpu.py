"""CPU: GpuIndex._row_ids, the one check of a host list of row ids (remove_rows, update_rows / the label scatter, get_rows).  No GPU and no
library call: the helper is pure numpy.  The ValueError texts are literals: callers and tests of the bindings match them."""
import numpy as np
import pytest

from lab_1806_vec_db_amd.index import GpuIndex


def _remove(rows):
    return GpuIndex._row_ids(rows, "remove_rows", sort=True)


CALLERS = {"remove_rows": _remove, "update_rows": GpuIndex._update_ids}
TEXTS = {
    "remove_rows": ("remove_rows: an array of integer row ids is needed", "remove_rows: negative row id", "remove_rows: duplicate row ids"),
    "update_rows": ("update_rows: an array of integer row ids is needed", "update_rows: negative row id", "update_rows: duplicate row ids"),
}


@pytest.mark.parametrize("name", ["remove_rows", "update_rows"])
def test_refusals_carry_the_callers_texts(name):
    ids = CALLERS[name]
    needed, negative, duplicate = TEXTS[name]
    for bad in ([True, False], np.array([True]), [1.0, 2.0], np.array([3.5]), np.array(2.0), np.array(True)):
        with pytest.raises(ValueError) as e:
            ids(bad)
        assert str(e.value) == needed, bad
    for bad in ([3, -1], np.array([-5], dtype=np.int64), np.array(-1), [-2, -2]):  # (negative is found before duplicate)
        with pytest.raises(ValueError) as e:
            ids(bad)
        assert str(e.value) == negative, bad
    for bad in ([4, 4], [9, 2, 7, 2], np.array([0, 5, 0], dtype=np.uint32), [2 ** 40, 1, 2 ** 40]):
        with pytest.raises(ValueError) as e:
            ids(bad)
        assert str(e.value) == duplicate, bad


@pytest.mark.parametrize("name", ["remove_rows", "update_rows"])
def test_accepted_shapes(name):
    ids = CALLERS[name]
    for empty in ([], (), np.zeros(0), np.zeros(0, dtype=np.bool_), np.zeros((0, 3), dtype=np.int32)):  # (nothing to check: any dtype)
        r = ids(empty)
        assert r.dtype == np.uint64 and r.shape == (0,)
    r = ids(np.array(7))  # 0-d: one row
    assert r.dtype == np.uint64 and r.tolist() == [7]
    r = ids(np.array([[9, 2], [7, 4]], dtype=np.int16))  # flattened
    assert r.dtype == np.uint64 and r.flags.c_contiguous
    assert r.tolist() == ([2, 4, 7, 9] if name == "remove_rows" else [9, 2, 7, 4])  # remove_rows sorts, update_rows keeps the order
    r = ids(np.array([2 ** 63, 1], dtype=np.uint64))
    assert r.tolist() == ([1, 2 ** 63] if name == "remove_rows" else [2 ** 63, 1])


def test_get_rows_allows_repeats():
    r = GpuIndex._row_ids([5, 1, 5], "get_rows", distinct=False)
    assert r.dtype == np.uint64 and r.tolist() == [5, 1, 5]
    for bad, text in (([0.5], "get_rows: an array of integer row ids is needed"), ([True], "get_rows: an array of integer row ids is needed"),
                      ([1, -1], "get_rows: negative row id")):
        with pytest.raises(ValueError) as e:
            GpuIndex._row_ids(bad, "get_rows", distinct=False)
        assert str(e.value) == text
