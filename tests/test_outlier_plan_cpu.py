"""CPU: vdb_outlier_plan (host only; csrc/outlier_plan.hpp) against its layout restated by hand, the lane-group widths, and every refusal."""
import ctypes as C

import pytest

import lab_1806_vec_db_amd as vdb
from lab_1806_vec_db_amd import _lib as L

FILL = 2**63 + 5
CASES = (  # (n, dim, u8, masked, m, k, chunk) -> (chunks, last, kk, group, graph = 8 m k, scratch = graph + 4 m + 12 n + chunk x (12 kp + 8) + queries) | the refusal
    ((300, 5, 0, 0, 300, 20, 64), (5, 44, 20, 32, 48000, 48000 + 1200 + 3600 + 64 * 260)),
    ((300, 5, 0, 1, 101, 200, 64), (2, 37, 100, 0, 161600, 161600 + 404 + 3600 + 64 * 1220 + 64 * 5 * 4)),
    ((100000, 8, 0, 0, 100000, 1023, 2**20), (5, 12620, 1023, 0, 818400000, 818400000 + 400000 + 1200000 + 21845 * 12296)),  # 256 MiB / (1024 x 12 B) lists
    ((1, 4, 0, 0, 1, 3, 16384), (1, 1, 0, 4, 24, 24 + 4 + 12 + 20)),
    ((10, 4, 0, 1, 0, 5, 100), (0, 0, 0, 8, 0, 120)),
    ((1000, 8, 0, 0, 1000, 0, 4096), "k must be"), ((1000, 8, 0, 0, 1000, 1024, 4096), "k must be"), ((1000, 8, 1, 0, 1000, 5, 4096), "f32 rows"),
    ((2**32, 8, 0, 0, 2**32, 5, 4096), "2^32 rows"), ((1000, 8, 0, 0, 1000, 5, 0), "flat_dup_chunk"), ((1000, 8, 0, 0, 1000, 5, 2**20 + 1), "flat_dup_chunk"),
    ((1000, 8, 0, 1, 1001, 5, 4096), "allowed rows"), ((1000, 8, 0, 0, 999, 5, 4096), "allowed rows"))


@pytest.mark.parametrize("args,want", CASES, ids=[str(w) for _, w in CASES])
def test_plan_and_refusals(args, want):
    out = C.c_uint64(FILL), C.c_uint64(FILL), C.c_uint64(FILL), C.c_uint32(77), C.c_uint64(FILL), C.c_uint64(FILL)
    st = L.load().vdb_outlier_plan(*args, *(C.byref(o) for o in out))
    if isinstance(want, str):  # a refusal leaves the outputs alone
        assert st == 1 and tuple(o.value for o in out) == (FILL, FILL, FILL, 77, FILL, FILL) and want in L.load().vdb_last_error().decode()
    else:
        assert st == 0 and tuple(o.value for o in out) == want
        n, dim, u8, masked, m, k, chunk = args
        assert vdb.GpuIndex.outlier_plan(n, dim, k, m if masked else None, chunk, bool(u8)) == want


def test_lane_group_widths():
    """pow2ceil(k) lanes per source row while a wave holds them; beyond 64 a wave per row (0)"""
    want = {1: 1, 2: 2, 3: 4, 20: 32, 32: 32, 33: 64, 63: 64, 64: 64, 65: 0, 200: 0}
    assert {k: vdb.GpuIndex.outlier_plan(5000, 16, k)[3] for k in want} == want
