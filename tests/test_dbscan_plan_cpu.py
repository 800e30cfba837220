"""CPU: vdb_dbscan_plan (host only; csrc/dbscan_plan.hpp) against its layout restated by hand, and every refusal."""
import ctypes as C
import math

import pytest

import lab_1806_vec_db_amd as vdb
from lab_1806_vec_db_amd import _lib as L

FILL = 2**63 + 5
CASES = (  # (n, dim, u8, masked, m, eps, min_samples, chunk) -> (chunks, last, gather, scratch: 13 B per row + radii + limits + 64 + queries) | the refusal
    ((300, 5, 0, 0, 300, 0.5, 1, 64), (5, 44, 0, 13 * 300 + 256 + 8 * 65 + 64)),
    ((300, 5, 0, 1, 101, math.inf, 2**32 - 1, 64), (2, 37, 1, 13 * 300 + 256 + 8 * 65 + 64 + 64 * 5 * 4)),
    ((65, 960, 1, 0, 65, -1.0, 5, 16384), (1, 65, 1, 13 * 65 + 264 + 8 * 66 + 64 + 65 * 960 * 4)),
    ((2**32 - 1, 8, 0, 1, 0, 0.5, 5, 2**20), (0, 0, 1, 13 * (2**32 - 1) + 8 + 64)),
    ((1000, 8, 0, 0, 1000, math.nan, 5, 4096), "NaN"), ((1000, 8, 0, 0, 1000, 0.5, 0, 4096), "min_samples"),
    ((1000, 8, 0, 0, 1000, 0.5, 2**32, 4096), "min_samples"), ((2**32, 8, 0, 0, 2**32, 0.5, 5, 4096), "2^32 rows"),
    ((1000, 8, 0, 0, 1000, 0.5, 5, 0), "flat_dup_chunk"), ((1000, 8, 0, 0, 1000, 0.5, 5, 2**20 + 1), "flat_dup_chunk"),
    ((1000, 8, 0, 1, 1001, 0.5, 5, 4096), "allowed rows"), ((1000, 8, 0, 0, 999, 0.5, 5, 4096), "allowed rows"))


@pytest.mark.parametrize("args,want", CASES, ids=[str(w) for _, w in CASES])
def test_plan_and_refusals(args, want):
    out = C.c_uint64(FILL), C.c_uint64(FILL), C.c_int(77), C.c_uint64(FILL)
    st = L.load().vdb_dbscan_plan(*args, *(C.byref(o) for o in out))
    if isinstance(want, str):  # a refusal leaves the outputs alone
        assert st == 1 and tuple(o.value for o in out) == (FILL, FILL, 77, FILL) and want in L.load().vdb_last_error().decode()
    else:
        assert st == 0 and tuple(o.value for o in out) == want
        n, dim, u8, masked, m, eps, ms, chunk = args
        assert vdb.GpuIndex.dbscan_plan(n, dim, eps, ms, m if masked else None, chunk, bool(u8)) == want[:2] + (bool(want[2]), want[3])
