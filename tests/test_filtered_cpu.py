"""CPU: the host side of the filtered Flat search -- pack_mask (the bit words of a row mask) and the new C ABI names: exported by
libvdbhip.so and bound in the ctypes table with the arity include/vdbhip.h declares."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

NEW = ("vdb_mask_create", "vdb_mask_count", "vdb_mask_destroy", "vdb_flat_knn_filtered", "vdb_flat_knn_filtered_device",
       "vdb_flat_range_filtered")


def test_pack_mask_bool_and_ids_agree():
    from lab_1806_vec_db_amd.index import pack_mask

    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 130, 1000):
        allow = rng.random(n) < 0.4
        w = pack_mask(allow, n)
        assert w.dtype == np.uint64 and w.shape == ((n + 63) // 64,)
        assert np.array_equal(w, pack_mask(np.flatnonzero(allow), n))
        assert np.array_equal(w, pack_mask([int(i) for i in np.flatnonzero(allow)][::-1], n))  # any order, a plain list
        for i in range(n):
            assert bool((int(w[i >> 6]) >> (i & 63)) & 1) == bool(allow[i])
        assert sum(bin(int(x)).count("1") for x in w) == int(allow.sum())


def test_pack_mask_bits_past_n_are_clear():
    from lab_1806_vec_db_amd.index import pack_mask

    for n in (1, 5, 63, 65, 127):
        w = pack_mask(np.ones(n, dtype=np.bool_), n)
        assert sum(bin(int(x)).count("1") for x in w) == n
        assert int(w[-1]) >> (((n - 1) & 63) + 1) == 0
    assert pack_mask(np.ones(64, dtype=np.bool_), 64)[0] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert pack_mask([], 0).shape == (0,) and pack_mask(np.zeros(0, dtype=np.bool_), 0).shape == (0,)
    assert not pack_mask([], 70).any()
    assert np.array_equal(pack_mask([3, 3, 69], 70), np.array([8, 32], dtype=np.uint64))  # duplicates are one bit


def test_pack_mask_rejects_bad_input():
    from lab_1806_vec_db_amd.index import pack_mask

    with pytest.raises(ValueError):
        pack_mask([0, 10], 10)
    with pytest.raises(ValueError):
        pack_mask([-1], 10)
    with pytest.raises(ValueError):
        pack_mask(np.ones(9, dtype=np.bool_), 10)
    with pytest.raises(ValueError):
        pack_mask([0.5], 10)


def test_new_names_exported_and_bound():
    from lab_1806_vec_db_amd import _lib

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as G

    lib = _lib.load()
    arity = {name: len(params) for name, _, params in G.c_decls()}
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by libvdbhip.so"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
        assert name in arity, f"{name} is not declared in include/vdbhip.h"
        assert len(_lib.SIGNATURES[name]) == arity[name], name


def test_python_surface():
    import inspect

    import lab_1806_vec_db_amd as vdb
    from lab_1806_vec_db_amd.vecdb import VecDB

    assert hasattr(vdb, "RowMask") and hasattr(vdb, "pack_mask")
    for m in ("make_mask", "flat_knn_filtered"):
        assert hasattr(vdb.GpuIndex, m)
    assert "mask" in inspect.signature(vdb.GpuIndex.range_search).parameters
    assert "filter" in inspect.signature(VecDB.search).parameters
    assert "filter" in inspect.signature(VecDB.search_within).parameters
