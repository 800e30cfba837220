"""CPU: the exact Flat range search is declared, exported and bound (vdb_flat_range, vdb_flat_range_device, vdb_range_lims,
vdb_range_copy, vdb_range_destroy); without a device the call fails loudly (no CPU fallback); destroying NULL is fine."""
import ctypes as C

import numpy as np
import pytest

NAMES = ("vdb_flat_range", "vdb_flat_range_device", "vdb_range_lims", "vdb_range_copy", "vdb_range_destroy")


def test_range_symbols_exported_and_bound():
    from lab_1806_vec_db_amd import _lib

    lib = _lib.load()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert len(_lib.SIGNATURES["vdb_flat_range"]) == 7 and len(_lib.SIGNATURES["vdb_flat_range_device"]) == 8


def test_range_surface_exists():
    import lab_1806_vec_db_amd as vdb

    assert callable(vdb.GpuIndex.range_search) and callable(vdb.GpuIndex.range_search_device)
    assert callable(vdb.VecDB.search_within)


def test_range_destroy_null_and_null_arguments():
    from lab_1806_vec_db_amd import _lib

    lib = _lib.load()
    assert lib.vdb_range_destroy(None) == 0
    lims = np.zeros(1, dtype=np.uint64)
    assert lib.vdb_range_lims(None, lims.ctypes.data_as(_lib.u64p)) != 0  # an error through vdb_last_error, never an abort
    assert b"null" in lib.vdb_last_error()
    h = C.c_void_p()
    q = np.zeros(4, dtype=np.float32)
    assert lib.vdb_flat_range(None, q.ctypes.data_as(_lib.f32p), 1, 4, q.ctypes.data_as(_lib.f32p), 0, C.byref(h)) != 0
    assert h.value is None


def test_range_no_cpu_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import lab_1806_vec_db_amd as vdb

    with pytest.raises(vdb.VdbError):
        vdb.GpuIndex(8, "l2sqr").range_search(np.zeros(8, np.float32), 1.0)
    db = vdb.VecDB()
    with pytest.raises(vdb.VdbError):
        db.create_table_if_not_exists("t", 8, "l2sqr")
        db.search_within("t", np.zeros(8, np.float32), 1.0)
